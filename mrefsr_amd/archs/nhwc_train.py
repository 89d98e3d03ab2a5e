"""Channels-last TRAINING engine: the autograd side of archs/nhwc.py.

The reference trains net_g with torch.autograd over NCHW tensors (multi_ref_restoration_model.py:197-279: forward,
``l_pix.backward()``, Adam step); on ROCm that is one MIOpen call per convolution and direction plus separate bias /
activation / residual / concatenation kernels (2 200 launches per step at BASELINE configs[2]'s per-GPU shape).  Here the
same graph is recorded over [N,H,W,C] tensors with one autograd node per FUSED launch of the inference engine:

  _Conv          conv_nhwc (bias, broadcast pre-activation term, LeakyReLU / ReLU / PReLU, residual, PixelShuffle, two-source
                 concatenation fused) -- backward: ONE pass for the activation derivative + bias gradient (+ PReLU weight
                 gradient) + max |g| (mrefsr_act_bwd_nhwc_f32), the input gradients as conv_nhwc launches on the point-mirrored,
                 transposed weights (dgrad of a stride-1 'same' convolution IS such a convolution), the weight gradient on
                 csrc/wgrad.hip (conv_wgrad3x3 / conv_wgrad1x1, on the same storage: no transposes)
  _ResBlock      x + conv2(relu(conv1(x))) as one node: the skip's gradient rides on conv1's input-gradient launch
  _ResChain      a trunk of such blocks as one node (RESCHAIN; RESBLOCK alone records them one by one): per block two input-gradient
                 launches that carry the ReLU mask, the skip add, the bias gradients and max |g| (mrefsr_conv_nhwc_bwd_f32), all
                 weight gradients of the trunk as batched launches at the end (mrefsr_conv_wgrad3x3_batch_f32)
  _ConvDynAgg    conv_offset_mask + DynAgg glue (mrefsr_conv_dynagg_f32) -- backward through mrefsr_dynagg_prep_bwd_f32
  _Dcn           fused gather + MFMA deformable convolution on channels-last features (mrefsr_dcn_fwd_f32) with its LeakyReLU
                 -- backward: two fused launches (dcn_bwd_data: columns gradient with the offset / mask / input gradients as its
                 epilogue; dcn_bwd_weight: columns re-gathered inside the GEMM), no C*9*H*W buffer
  _Attention     mrefsr_mrattn_fwd_nhwc_f32 / mrefsr_mrattn_bwd_nhwc_f32 (softmax recomputed, nothing extra saved); with a
                 per-sample reference mask the _masked_ forms of both
  _Modulate      refs * sigmoid(mul) * 2 + add, one pass each way
  _Pad, _Crop    MRAPAFusion's reflect pad to a multiple of 4 and the crop back (csrc/pad.hip), one pass each way
  _VggLoss       the VGG of PerceptualLoss (losses/): output and GT as one batch forward, input gradients of the output image
                 backward (csrc/percep.hip: pooling, tap criterion, Gram matrices, image packing backward)
  _VggContextual the same VGG stack for ContextualLoss: per tap the all-pairs similarity, its statistics and their backward on
                 csrc/contextual.hip; with the CoBi options also a tap on RGB patches of the images and taps on a strided sub-grid

Arithmetic: forward and input-gradient convolutions run the fp16 two-term split (terms 16, three products; FWD_TERMS /
BWD_TERMS) on weights packed with a cached power-of-two scale (_wscale, watched by check_scales()); an input-gradient launch
scales its incoming gradient by the power of two that the launch before it derived from max |g| (gradients of 1e-8 are far below
the fp16 normal range).  All packed copies are refreshed by ONE multi-tensor launch per step (begin_step()).

The range-free re-run (hip.range_free(): an activation or weight left the fp16 range, the model repeats the batch) uses instead:
the bf16 three-term split (terms 6: fp32-equivalent, no range limit) for every convolution, _fwd_pack / _bwd_pack / _vgg_pack
choosing it -- also for a weight without a scale (all zero); the generic forms of _wgrad (a split-K bmm for 1x1, MIOpen's
channels-last weight gradient for 3x3) per convolution, also inside _ResChain; the four-launch block backward in _ResChain; the
unfused PReLU in conv(); and for the DCN, as for shapes its fused kernels refuse, im2col / col2im with two library GEMMs
(ops/dcn/deform_conv.py, fused=False).

Gradients match the reference's own optimisation step to the fingerprints of tests/golden/e2e_c2.npz
(tests/test_configs_gpu.py).  ``ENABLED`` is flipped by tests/ only (generic NCHW autograd forms as the comparison).
"""
import collections
import os
import weakref

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import hip
from ..param_cache import Packed, param_stamp

# MIOpen's channels-last kernels for the generic weight gradients of _wgrad (read once by torch, at its first MIOpen convolution)
os.environ.setdefault('PYTORCH_MIOPEN_SUGGEST_NHWC', '1')

ENABLED = True
TERMS = 6
# Forward convolutions on the fp16 two-term split (3 products instead of 6: the small maps of a training step are bound by
# the serial MFMA chain of one block).  Its weight scale 2^s (max|w| 2^s in [2^13, 2^14)) comes from a readback of the
# weight's amax when a parameter is first seen -- not per step: weights drift slowly, and check_scales() (one multi-tensor
# launch per step, no synchronisation) raises the library's range flag if a weight has grown past the cached headroom (4x),
# upon which the model re-runs the step on the range-free kernels and the scales are taken afresh.
FWD_TERMS = int(os.environ.get('MREFSR_TRAIN_FWD_TERMS', '16'))
REFRESH = 50          # steps between full refreshes of the cached scales (one readback of all amaxes)
_Scale = collections.namedtuple('_Scale', 'ref scale limit')


def _scale_of(amax):
    """2^s with amax * 2^s in [2^13, 2^14); None for an (almost) all-zero weight (conv_offset_mask right after its zero
    initialisation): that convolution runs the range-free split until a refresh finds it grown"""
    import math
    if not (amax > 2.0 ** -40 and math.isfinite(amax)):
        return None
    return 2.0 ** (13 - math.floor(math.log2(amax)))


def _scale_entry(weight, amax):
    s = _scale_of(amax)
    return _Scale(weakref.ref(weight), s, 60000.0 / s if s else float('inf'))


class _WeightScales:
    """The scale of every training weight, its limit 60000 / scale and the cadence of their refresh, by the parameter's storage (the
    same for every handle autograd hands back).  Of param_stamp() an entry asks only ``alive``: a scale outlives versions on purpose."""

    def __init__(self):
        self.entries, self.epoch, self.checks, self.lim, self.lim_key = {}, 0, 0, None, None

    def has(self, weight):
        return (weight.data_ptr(), weight.numel()) in self.entries

    def get(self, weight):
        key = (weight.data_ptr(), weight.numel())
        hit = self.entries.get(key)
        if hit is not None and param_stamp(hit.ref()).alive:
            return hit.scale
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('nhwc_train: the fp16 weight scale of a parameter is not cached yet (first use, or its holder was freed) and '
                               'deriving it needs a readback, which a hipGraph capture cannot contain: run one eager step first')
        hit = self.entries[key] = _scale_entry(weight, float(weight.detach().abs().max().item()))
        self.epoch += 1
        return hit.scale

    def reset(self):
        self.entries.clear()
        self.epoch += 1

    def check(self):
        """once per training step, before the forward pass: every cached scale still leaves max|w| * scale inside the fp16 range, else the
        range flag of hip.conv_range_tripped() is raised (device side: no synchronisation).  Every REFRESH-th call: all scales anew."""
        live = [(k, w) for k, w in ((k, e.ref()) for k, e in self.entries.items()) if param_stamp(w).alive]
        self.entries = {k: self.entries[k] for k, _ in live}
        if not live:
            return
        amax = torch.stack(torch._foreach_norm([w.detach() for _, w in live], float('inf')))
        self.checks += 1
        if self.checks % REFRESH == 0:
            fresh = {k: _scale_entry(w, a) for (k, w), a in zip(live, amax.tolist())}
            self.epoch += any(e.scale != self.entries[k].scale for k, e in fresh.items())
            self.entries = fresh
            return
        if self.lim_key != (self.epoch, len(live)):
            self.lim_key, self.lim = (self.epoch, len(live)), torch.tensor([self.entries[k].limit for k, _ in live], device=amax.device)
        hip._range_flag(amax.device).bitwise_or_((amax > self.lim).any().to(torch.int32))


_scales = _WeightScales()
_wscale, reset_scales, check_scales = _scales.get, _scales.reset, _scales.check


def scale_epoch():
    return _scales.epoch


def _fwd_terms():
    return TERMS if (FWD_TERMS != 16 or hip.is_range_free()) else 16


# Input-gradient convolutions on the same three-product mode: the output gradients of an L1-trained network sit around
# 1e-6..1e-9, far below the fp16 normal range, so the backward glue kernel also returns max |g| and the convolution kernel
# scales its input by the power of two that brings that maximum to [2^13, 2^14) (mrefsr_conv_nhwc_scaled_f32; exact both ways)
BWD_TERMS = int(os.environ.get('MREFSR_TRAIN_BWD_TERMS', '16'))


_PACK_KEEP = 4     # refreshes an unused entry survives (validation passes, a second network)
_PackKey = collections.namedtuple('_PackKey', 'what wscale')   # what: (data_ptr, numel, shape, slice, terms, operator)


class _PackTable:
    """Packed copies of one device's training weights.  A parameter changes once per step (optimizer_g.step(), ref
    multi_ref_restoration_model.py:277) and is used by two launches (forward operator, input-gradient operator): 346 packing launches
    of ~4 us per step.  The copies live in persistent buffers instead (entries: _PackKey -> Packed), and ONE multi-tensor launch
    (mrefsr_conv_pack_weights_multi_f32, a job table in device memory) refreshes all of them: at begin_step() -- called by the model
    at the top of every optimisation step, also inside the hipGraph capture -- or at the first lookup that finds a copy older than
    its parameter (callers that drive net_g without the model).  A new (weight, slice, arithmetic) is packed alone once and joins the
    next refresh's table.  Keyed by the parameter's STORAGE, not by id() as hip's inference cache: autograd hands back new Python
    handles.  Stamps carry the capture epoch.  ``frozen``: copies of weights that are never stepped (the perceptual VGG): never
    in the job table, no _PACK_KEEP, re-made alone when the stamp moves (load_state_dict)."""

    def __init__(self, device):
        self.device, self.frozen = device, {}
        self.reset()

    def reset(self):
        self.entries, self.table, self.rows, self.dirty, self.refreshes = {}, None, [], True, 0

    def refresh(self):
        """repack every live entry in one launch; False when that takes a new job table (an upload) inside a hipGraph capture"""
        cap, epoch = hip.capture_epoch()
        # dead: the parameter is gone, its storage was replaced (`p.data = ...`, `.to()`: the job row still holds the old address),
        # or nothing has asked for the copy for _PACK_KEEP refreshes
        now = {k: param_stamp(e.ref()) for k, e in self.entries.items()}
        dead = [k for k, e in self.entries.items() if not now[k].alive or now[k].ptr != e.stamp.ptr or self.refreshes - e.last_used > _PACK_KEEP]
        if (dead or self.dirty) and cap:
            return False
        for k in dead:
            del self.entries[k]
        self.refreshes += 1
        if dead or self.dirty:
            self.rows = list(self.entries.values())
            self.table = hip.conv_pack_table([e.job for e in self.rows], self.device) if self.rows else None
            self.dirty = False
        if self.rows:
            hip.conv_pack_multi(self.table, len(self.rows))
            for e in self.rows:
                e.stamp = param_stamp(e.ref(), epoch)
        return True

    def get(self, weight, cin_slice, terms, dgrad=False, wscale=1.0):
        """hip.conv_pack_view(weight, cin_slice, terms, dgrad, wscale) from the step's refreshed copies"""
        cap, epoch = hip.capture_epoch()
        what = (weight.data_ptr(), weight.numel(), tuple(weight.shape), cin_slice, terms, dgrad)
        e = self.entries.get((what, wscale))
        now = None if e is None else param_stamp(e.ref(), epoch)
        if now is not None and now.alive:
            e.last_used = self.refreshes
            if e.stamp != now and not (self.refresh() and e.stamp == now):
                hip.conv_pack_one(e.job)   # (table being rebuilt under capture, or the entry is not in the table yet): this copy alone
                e.stamp = now
            return e.packed
        pw, job = hip.conv_pack_plan(weight, cin_slice, terms, dgrad, wscale)
        hip.conv_pack_one(job)
        if not cap:   # copies of the same (weight, slice, arithmetic, operator) at a superseded scale: nobody reads them again, and a
            for k in [k for k in self.entries if k.what == what and k.wscale != wscale]:   # repack could raise the range flag for them
                del self.entries[k]
        self.entries[_PackKey(what, wscale)] = Packed(weight, pw, param_stamp(weight, epoch), job, self.refreshes)
        self.dirty = True
        return pw

    def get_frozen(self, weight, cin_slice, terms, dgrad, wscale):
        key = (weight.data_ptr(), weight.numel(), cin_slice, terms, dgrad, wscale)
        e = self.frozen.get(key)
        if e is None or param_stamp(e.ref()) != e.stamp:
            for k in [k for k, o in self.frozen.items() if not param_stamp(o.ref()).alive]:
                del self.frozen[k]
            pw = hip.conv_pack_view(weight.detach(), cin_slice, terms, dgrad=dgrad, wscale=wscale)
            e = self.frozen[key] = Packed(weight, pw, param_stamp(weight))
        return e.packed


_packs = {}        # device index -> _PackTable


def _packed(weight, cin_slice, terms, dgrad=False, wscale=1.0, frozen=False):
    t = _packs.get(weight.device.index) or _packs.setdefault(weight.device.index, _PackTable(weight.device))
    return (t.get_frozen if frozen else t.get)(weight, cin_slice, terms, dgrad, wscale)


def begin_step(device=None):
    """top of an optimisation step: refresh every packed weight copy (one launch per device that has any)"""
    for idx in list(_packs) if device is None else [torch.device(device).index]:
        if idx in _packs and _packs[idx].entries:
            _packs[idx].refresh()


def reset_packs():
    for t in _packs.values():
        t.reset()


def capture_state():
    """(objects, addresses) a hipGraph captured now has baked in from this module's caches: the job table of the multi-tensor pack
    launch, every packed copy and the parameter each one is made from.  The model keeps the objects alive as long as the graph and
    compares the addresses before every replay (a table rebuilt by an eager pass in between, a parameter whose storage was
    replaced: the graph would read freed memory)."""
    objs, ptrs = [], []
    for _, t in sorted(_packs.items()):
        objs.append((t.table, list(t.rows)))
        ptrs.append(t.table.data_ptr() if t.table is not None else 0)
        for e in t.rows:
            now = param_stamp(e.ref())
            ptrs.append((e.packed.data.data_ptr(), now.ptr if now.alive else -1))
    ptrs.append(hip.capture_ptrs())   # the capture's cached scratch, ticket words and zero chunks: a regrown one has moved
    return objs, tuple(ptrs)


def _pack(weight, cin_slice, dgrad=False, frozen=False):
    """(packed forward / input-gradient operator, terms): the fp16 two-term split with the weight's cached scale (FWD_TERMS /
    BWD_TERMS 16, outside hip.range_free(), a weight that has a scale), else the range-free split"""
    want16 = (BWD_TERMS == 16 and not hip.is_range_free()) if dgrad else _fwd_terms() == 16
    ws = _wscale(weight) if want16 else None
    if ws is not None:
        return _packed(weight, cin_slice, 16, dgrad, ws, frozen), 16
    return _packed(weight, cin_slice, TERMS, dgrad, frozen=frozen), TERMS


def _fwd_pack(weight, cin_slice):
    return _pack(weight, cin_slice)


def _bwd_pack(weight, cin_slice):
    return _pack(weight, cin_slice, dgrad=True)


def _unshuffle(t):
    """inverse of PixelShuffle(2) on channels-last storage: [N,2H,2W,C] -> [N,H,W,4C] (channel 4c + 2i + j)"""
    n, h2, w2, c = t.shape
    return t.view(n, h2 // 2, 2, w2 // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(n, h2 // 2, w2 // 2, 4 * c)


def _wgrad(g_pre, cout, x, cin, k, amax=None):
    """d loss / d weight [cout,cin,k,k] from channels-last storage (g_pre [N,H,W,>=cout], x [N,H,W,>=cin]): the library's own
    kernels (csrc/wgrad.hip); the generic forms below serve what those refuse, a batch that is being re-run on the range-free path
    (an activation left the fp16 range) -- see INTEGRATION.md"""
    if k == 3 and amax is not None and not hip.is_range_free():
        return hip.conv_wgrad3x3(x, g_pre, cin, cout, amax)
    if k == 1 and amax is not None and not hip.is_range_free():
        return hip.conv_wgrad1x1(x, g_pre, cin, cout, amax)
    if k == 1:
        # (range-free re-runs) a plain GEMM over the pixels, g^T [cout, P] . x [P, cin], on the tensors as they lie; K = P is ~10^5 against M, N of a
        # few hundred, so it is split into S batches (a library GEMM has no split-K for this shape: 4x slower) and the
        # S partial results are added
        g2, x2 = g_pre.reshape(-1, g_pre.shape[3]), x.reshape(-1, x.shape[3])
        p_ = g2.shape[0]
        split = next((d for d in (128, 100, 64, 50, 40, 32, 25, 20, 16, 10, 8, 5, 4, 2) if p_ % d == 0 and p_ // d >= 256), 1)
        g3 = g2.view(split, p_ // split, g2.shape[1])[:, :, :cout]
        x3 = x2.view(split, p_ // split, x2.shape[1])[:, :, :cin]
        return torch.bmm(g3.transpose(1, 2), x3).sum(0).view(cout, cin, 1, 1)
    g = g_pre.permute(0, 3, 1, 2)
    xi = x.permute(0, 3, 1, 2)
    if g.shape[1] != cout:
        g = g[:, :cout]
    if xi.shape[1] != cin:
        xi = xi[:, :cin]
    w = torch.empty((cout, cin, k, k), device=x.device, dtype=x.dtype).contiguous(memory_format=torch.channels_last)
    _, gw, _ = torch.ops.aten.convolution_backward(g, xi, w, None, [1, 1], [k // 2, k // 2], [1, 1], False, [0, 0], 1, [False, True, False])
    return gw


class _Conv(Function):
    """out = act(conv(cat[x1, x2]; weight[:, a:b]) + bias + pre) + residual, optionally through PixelShuffle(2)"""

    @staticmethod
    def forward(ctx, x1, x2, weight, bias, prelu_w, pre, residual, slope, epilogue, cin_slice):
        co, ci, k, _ = weight.shape
        act = 2 if prelu_w is not None else (1 if slope is not None else 0)
        if act and residual is not None:
            raise NotImplementedError('nhwc_train: activation followed by a residual add in one launch has no fused backward')
        if cin_slice is not None and x2 is not None:
            raise NotImplementedError('nhwc_train: cin_slice with a second source')
        weight = weight.contiguous()
        a, b = cin_slice if cin_slice is not None else (0, ci)
        packed, _ = _fwd_pack(weight, (a, b))
        out = hip.conv_nhwc(x1, packed, bias, co, k, x2=x2, pre=pre, residual=residual, act=act != 0, slope=slope if act == 1 else 0.0,
                            slope_ptr=prelu_w, epilogue=epilogue)
        ctx.meta = (act, slope, epilogue, (a, b), k, bias is not None, 0 if pre is None else pre.shape[0])
        ctx.save_for_backward(x1, x2, weight, prelu_w, out if act else None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x1, x2, weight, prelu_w, out = ctx.saved_tensors
        act, slope, epilogue, (a, b), k, has_bias, pre_n = ctx.meta
        need = ctx.needs_input_grad
        co = weight.shape[0]
        g = g.contiguous()
        g_res = g if need[6] else None
        if epilogue == 2:
            g = _unshuffle(g)
            if act:
                out = _unshuffle(out)
        dgrad = need[0] or (x2 is not None and need[1])
        g_pre, g_bias, g_slope, amax = hip.act_bwd_nhwc(g, out, act, slope if act == 1 else 0.0, prelu_w, want_bias=has_bias and need[3],
                                                        want_amax=True) if (dgrad or need[2]) else \
            hip.act_bwd_nhwc(g, out, act, slope if act == 1 else 0.0, prelu_w, want_bias=has_bias and need[3]) + (None,)
        n, h, w, _ = g_pre.shape
        g_x1 = g_x2 = g_w = g_p = None
        c1 = x1.shape[3] if x2 is not None else b - a
        if need[0]:
            if x1.shape[3] != c1 or x1.shape[0] != n:
                raise NotImplementedError('nhwc_train: gradient of a channel-padded / batch-broadcast input')
            pk, terms = _bwd_pack(weight, (a, a + c1))
            g_x1 = hip.conv_nhwc(g_pre, pk, None, c1, k, in_amax=amax if terms == 16 else None)
        if x2 is not None and need[1]:
            if x2.shape[0] != n:
                raise NotImplementedError('nhwc_train: gradient of a batch-broadcast input')
            pk, terms = _bwd_pack(weight, (c1, c1 + x2.shape[3]))
            g_x2 = hip.conv_nhwc(g_pre, pk, None, x2.shape[3], k, in_amax=amax if terms == 16 else None)
        if need[2]:
            gw1 = _wgrad(g_pre, co, x1, c1, k, amax)
            if x2 is not None:
                g_w = torch.cat([gw1, _wgrad(g_pre, co, x2, x2.shape[3], k, amax)], 1)
            elif (a, b) == (0, weight.shape[1]):
                g_w = gw1
            else:
                g_w = torch.zeros_like(weight)
                g_w[:, a:b] = gw1
        if pre_n and need[5]:
            gp = g_pre if g_pre.shape[3] == co else g_pre[..., :co]
            g_p = gp.reshape(n // pre_n, pre_n, h, w, co).sum(0) if pre_n != n else gp
        return g_x1, g_x2, g_w, g_bias, g_slope, g_p, g_res, None, None, None


def _resblock_fwd(x, w1, b1, w2, b2):
    """(t, out) = (relu(conv1(x)), x + conv2(t)): the two launches of a residual block"""
    pk1, _ = _fwd_pack(w1, (0, w1.shape[1]))
    pk2, _ = _fwd_pack(w2, (0, w2.shape[1]))
    t = hip.conv_nhwc(x, pk1, b1, w1.shape[0], 3, act=True, slope=0.0)
    return t, hip.conv_nhwc(t, pk2, b2, w2.shape[0], 3, residual=x)


class _ResBlock(Function):
    """x + conv2(relu(conv1(x))) -- ResidualBlockNoBN with res_scale 1 (arch_util.py:45-70) -- as ONE autograd node: recorded as
    two _Conv nodes, autograd adds the two gradients of x (identity path and conv1's input gradient) in a launch of its own, 48
    times per trunk; here conv1's input-gradient convolution takes the incoming gradient as its fused residual term."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        w1, w2 = w1.contiguous(), w2.contiguous()
        t, out = _resblock_fwd(x, w1, b1, w2, b2)
        ctx.save_for_backward(x, t, w1, w2)
        ctx.has_bias = (b1 is not None, b2 is not None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, t, w1, w2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        c = w1.shape[0]
        g = g.contiguous()
        _, g_b2, _, amax2 = hip.act_bwd_nhwc(g, None, 0, want_bias=ctx.has_bias[1] and need[4], want_amax=True)
        pk, terms = _bwd_pack(w2, (0, c))
        g_t = hip.conv_nhwc(g, pk, None, c, 3, in_amax=amax2 if terms == 16 else None)
        g_w2 = _wgrad(g, w2.shape[0], t, c, 3, amax2) if need[3] else None
        g_pre, g_b1, _, amax1 = hip.act_bwd_nhwc(g_t, t, 1, 0.0, want_bias=ctx.has_bias[0] and need[2], want_amax=True)
        g_x = None
        if need[0]:
            pk, terms = _bwd_pack(w1, (0, w1.shape[1]))
            g_x = hip.conv_nhwc(g_pre, pk, None, w1.shape[1], 3, residual=g, in_amax=amax1 if terms == 16 else None)
        g_w1 = _wgrad(g_pre, c, x, w1.shape[1], 3, amax1) if need[1] else None
        return g_x, g_w1, g_b1, g_w2, g_b2


class _ResChain(Function):
    """A whole trunk of residual blocks (nn.Sequential of ResidualBlockNoBN, 16 per scale in MRAPARestorationNet) as ONE node:
    the input gradients run block by block as in _ResBlock, the 2 * n_blocks weight gradients -- which feed nothing inside
    backward -- are left for the end and run as one batched launch pair (mrefsr_conv_wgrad3x3_batch_f32): 2 launches instead of
    64 per trunk, and on the small maps the blocks of all 32 jobs fill the chip together instead of 80 at a time."""

    @staticmethod
    def forward(ctx, x, *params):
        nb = len(params) // 4
        saved = [x]
        for i in range(nb):
            t, x = _resblock_fwd(x, *params[4 * i:4 * i + 4])   # (reschain() admits square blocks of one width only)
            saved += [t, x]
        ctx.nb = nb
        ctx.save_for_backward(*saved[:-1], *params)     # x_0, (t_i, x_i+1) ... without the output
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        nb = ctx.nb
        acts, params = ctx.saved_tensors[:2 * nb], ctx.saved_tensors[2 * nb:]
        c = params[0].shape[0]
        g = g.contiguous()
        grads = [None] * (4 * nb)
        jobs_x, jobs_g, jobs_a, slots = [], [], [], []
        stats = None   # (bias gradient of conv2, max |g|) of the current g when the launch that produced it has already made them
        for i in reversed(range(nb)):
            w1, b1, w2, b2 = params[4 * i:4 * i + 4]
            x, t = acts[2 * i], acts[2 * i + 1]
            if stats is None:
                _, g_b2, _, amax2 = hip.act_bwd_nhwc(g, None, 0, want_bias=True, want_amax=True)
            else:
                g_b2, amax2 = stats
            pk2, terms2 = _bwd_pack(w2, (0, c))
            pk1, terms1 = _bwd_pack(w1, (0, c))
            if terms1 == 16 and terms2 == 16:
                # both element-wise passes of the block ride on the input-gradient launches: conv2's takes the ReLU mask from t and
                # leaves conv1's bias gradient and the scale of its own output; conv1's adds the skip and leaves the same for the
                # block above (mrefsr_conv_nhwc_bwd_f32) -- two launches per block instead of four, no extra pass over g
                g_pre, g_b1, amax1 = hip.conv_nhwc_bwd(g, pk2, c, 3, residual=t, residual_is_mask=True, in_amax=amax2)
                g_in, sb, sa = hip.conv_nhwc_bwd(g_pre, pk1, c, 3, residual=g, in_amax=amax1, want_stats=i > 0)
                stats = (sb, sa) if i > 0 else None
            else:
                g_t = hip.conv_nhwc(g, pk2, None, c, 3, in_amax=amax2 if terms2 == 16 else None)
                g_pre, g_b1, _, amax1 = hip.act_bwd_nhwc(g_t, t, 1, 0.0, want_bias=True, want_amax=True)
                g_in = hip.conv_nhwc(g_pre, pk1, None, c, 3, residual=g, in_amax=amax1 if terms1 == 16 else None)
                stats = None
            grads[4 * i + 1], grads[4 * i + 3] = g_b1, g_b2
            jobs_x += [t, x]
            jobs_g += [g, g_pre]
            jobs_a += [amax2, amax1]
            slots += [4 * i + 2, 4 * i]
            g = g_in
        if hip.is_range_free():
            for x_, g_, a_, s_ in zip(jobs_x, jobs_g, jobs_a, slots):
                grads[s_] = _wgrad(g_, c, x_, c, 3, a_)
        else:
            for k in range(0, len(jobs_x), 32):
                dw = hip.conv_wgrad3x3_batch(jobs_x[k:k + 32], jobs_g[k:k + 32], c, c, jobs_a[k:k + 32])
                for j, s_ in enumerate(slots[k:k + 32]):
                    grads[s_] = dw[j]
        return (g if ctx.needs_input_grad[0] else None, *grads)


class _ConvDynAgg(Function):
    """(feat [N,H,W,C], conv_offset_mask weight / bias, pre_offset) -> planar (offset, mask) for the DCN   ref :56-73"""

    @staticmethod
    def forward(ctx, feat, weight, bias, pre_offset, dg, abs_sum):
        weight = weight.contiguous()
        packed, _ = _fwd_pack(weight, None)
        offset, mask = hip.conv_dynagg(feat, packed, bias, pre_offset, dg, abs_sum)
        ctx.dg = dg
        ctx.save_for_backward(feat, weight, mask)
        return offset, mask

    @staticmethod
    @once_differentiable
    def backward(ctx, g_offset, g_mask):
        feat, weight, mask = ctx.saved_tensors
        co = weight.shape[0]
        if 27 * ctx.dg <= 256:   # channels-last result, bias gradient and max |g| from ONE pass (no transposing copy, no reduction pass)
            g_om, g_bias, amax = hip.dynagg_prep_bwd_nhwc(g_offset.contiguous(), g_mask.contiguous(), mask, ctx.dg, want_bias=ctx.needs_input_grad[2])
        else:
            g_om = hip.dynagg_prep_bwd(g_offset.contiguous(), g_mask.contiguous(), mask, ctx.dg)     # [N,27dg,H,W]
            g_om = g_om.permute(0, 2, 3, 1).contiguous()
            _, g_bias, _, amax = hip.act_bwd_nhwc(g_om, None, 0, want_bias=ctx.needs_input_grad[2], want_amax=True)
        g_feat = g_w = None
        if ctx.needs_input_grad[0]:
            pk, terms = _bwd_pack(weight, None)
            g_feat = hip.conv_nhwc(g_om, pk, None, feat.shape[3], 3, in_amax=amax if terms == 16 else None)
        if ctx.needs_input_grad[1]:
            g_w = _wgrad(g_om, co, feat, feat.shape[3], 3, amax)
        return g_feat, g_w, g_bias, None, None, None


class _Dcn(Function):
    """lrelu(DCNv2(x; offset, mask), act_slope) on channels-last x [N,H,W,C] -> [N,H,W,Co]; offset / mask planar"""

    @staticmethod
    def forward(ctx, x, offset, mask, weight, bias, dg, act_slope):
        out = hip.dcn_fwd(x, offset, mask, weight, bias, 1, 1, 1, 1, dg, act_slope, channels_last=True)
        ctx.dg, ctx.act_slope = dg, act_slope
        ctx.save_for_backward(x, offset, mask, weight, out if act_slope != 1.0 else None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from ..ops.dcn.deform_conv import _backward
        x, offset, mask, weight, out = ctx.saved_tensors
        g = g.contiguous()
        c, co = x.shape[3], weight.shape[0]
        ws = None if hip.is_range_free() else _wscale(weight)
        if ws is not None and c % 32 == 0 and c // ctx.dg in (8, 16, 32) and co % 16 == 0:
            # fused: d columns = W^T . g on the matrix pipe with the offset / mask / input gradients as its epilogue, d W with the
            # columns re-gathered inside the GEMM -- no C*9*H*W buffer, no library GEMM (deform_conv_cuda.cpp:571-685 as two launches)
            g_pre, g_bias, _, amax = hip.act_bwd_nhwc(g, out, 0 if out is None else 1, ctx.act_slope, want_bias=ctx.needs_input_grad[4], want_amax=True)
            need_x = ctx.needs_input_grad[0]
            gx = goff = gm = gw = None
            if need_x or ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
                pk = _packed(weight, None, 16, dgrad='T', wscale=ws)
                gx, goff, gm = hip.dcn_bwd_data(g_pre, x, offset, mask, pk, ctx.dg, g_amax=amax, need_grad_x=need_x)
                if gx is not None:
                    gx = gx.permute(0, 2, 3, 1).contiguous()
            if ctx.needs_input_grad[3]:
                gw = hip.dcn_bwd_weight(g_pre, x, offset, mask, co, ctx.dg, g_amax=amax)
            return gx, goff, gm, gw, g_bias, None, None
        g_pre, g_bias, _ = hip.act_bwd_nhwc(g, out, 0 if out is None else 1, ctx.act_slope, want_bias=ctx.needs_input_grad[4])
        ctx.stride, ctx.padding, ctx.dilation, ctx.groups, ctx.deformable_groups = 1, 1, 1, 1, ctx.dg
        gx, goff, gm, gw, _ = _backward(ctx, g_pre.permute(0, 3, 1, 2), x.permute(0, 3, 1, 2).contiguous(), offset, mask, weight,
                                        False, ctx.needs_input_grad[0], fused=False)   # (the fused kernels were refused above)
        if gx is not None:
            gx = gx.permute(0, 2, 3, 1).contiguous()
        return gx, goff, gm, gw, g_bias, None, None


class _Attention(Function):
    """softmax_t(<q, emb_t>) . ass_t per pixel on channels-last tensors (t-major references)   ref :321-335"""

    @staticmethod
    def forward(ctx, q, emb, ass, t, valid_bits=None):
        """valid_bits ([n] int32, bit t = reference t of the sample is present) or None: all present, the unmasked kernels"""
        ctx.t, ctx.valid_bits = t, valid_bits
        ctx.save_for_backward(q, emb, ass)
        if valid_bits is not None:
            return hip.mrattn_fwd_nhwc_masked(q, emb, ass, t, valid_bits)
        return hip.mrattn_fwd_nhwc(q, emb, ass, t)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        q, emb, ass = ctx.saved_tensors
        if ctx.valid_bits is not None:
            return hip.mrattn_bwd_nhwc_masked(q, emb, ass, g.contiguous(), ctx.t, ctx.valid_bits) + (None, None)
        return hip.mrattn_bwd_nhwc(q, emb, ass, g.contiguous(), ctx.t) + (None, None)


class _Modulate(Function):
    """refs * sigmoid(mul) * 2 + add   ref :343-345"""

    @staticmethod
    def forward(ctx, refs, mul, add):
        ctx.save_for_backward(refs, mul)
        return hip.attn_modulate_(refs, mul.clone(), add)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        refs, mul = ctx.saved_tensors
        g = g.contiguous()
        return hip.attn_modulate_bwd(g, refs, mul) + (g,)


class _Pad(Function):
    """bottom / right reflect pad of [N,H,W,C] by ph, pw in 0..3   ref :306-311"""

    @staticmethod
    def forward(ctx, x, ph, pw):
        ctx.pads = (ph, pw)
        return hip.reflect_pad_nhwc(x, ph, pw)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return hip.reflect_pad_bwd_nhwc(g.contiguous(), *ctx.pads), None, None


class _Crop(Function):
    """top-left h0 x w0 window of [N,H,W,C]   ref :348"""

    @staticmethod
    def forward(ctx, x, h0, w0):
        ctx.hw = tuple(x.shape[1:3])
        return hip.crop_nhwc(x, h0, w0)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return hip.crop_bwd_nhwc(g.contiguous(), *ctx.hw), None, None


# ---- perceptual / style loss (PerceptualLoss, losses.py:141-238 of the reference model's loss module) ----------------------------
POOL_PLANE = os.environ.get('MREFSR_PERCEP_POOL_PLANE', '0') == '1'   # 1: the forward stores the pool's arg-max plane
KEEP_TAPS = None   # tests/ set a list: every _VggLoss forward appends its [2B,h,w,c] tap features (sign decisions against fp64)


def _vgg_pack(weight, cin_slice, dgrad):
    """_pack for a frozen VGG convolution: the engine's training arithmetic on copies that stay out of the per-step refresh"""
    return _pack(weight, cin_slice, dgrad, frozen=True)


class VggLossPlan:
    """The tapped VGG stack of a PerceptualLoss as a list of convolution layers, each with the names of its ReLU / pool (if the
    stack reaches them) and which of conv / relu / pool are tapped: what _VggLoss runs"""

    def __init__(self, vgg_net, layer_weights, criterion, perceptual_weight, style_weight, norm_img):
        from torch import nn
        items = list(vgg_net._modules.items())
        self.layers = []
        for name, mod in items:
            if isinstance(mod, nn.Conv2d):
                self.layers.append(dict(conv=mod, names={'conv': name}))
            elif isinstance(mod, nn.ReLU):
                self.layers[-1]['names']['relu'] = name
            elif isinstance(mod, nn.MaxPool2d):
                self.layers[-1]['names']['pool'] = name
            else:
                raise NotImplementedError(f'perceptual loss: VGG layer {name} ({type(mod).__name__}) has no kernel here')
        self.taps = []   # (layer index, 'conv' | 'relu' | 'pool', weight) in network order
        for i, l in enumerate(self.layers):
            for kind in ('conv', 'relu', 'pool'):
                nm = l['names'].get(kind)
                if nm is not None and nm in layer_weights:
                    self.taps.append((i, kind, float(layer_weights[nm])))
        if len(self.taps) != len(layer_weights) or len(self.taps) > 8:   # (perceptual + style jobs of one criterion launch: <= 16)
            raise NotImplementedError(f'perceptual loss: layer_weights {sorted(layer_weights)} (at most 8 taps, all inside the VGG stack)')
        self.crit, self.pw, self.sw, self.norm_img = criterion, float(perceptual_weight), float(style_weight), bool(norm_img)


def _vgg_stack_forward(plan, img, mean, std):
    """the tapped VGG stack on the images img [N,3,H,W] -> (tap features [N,h,w,c] in the order of plan.taps, what the backward
    needs per layer: (mask source, its ReLU not applied yet, pool plane, pool input shape))"""
    h = hip.image_to_nhwc4(img, mean, std, plan.norm_img)
    saved = []
    tapv = {}           # (layer, kind) -> [N,h,w,c] tensor
    last = len(plan.layers) - 1
    tapped = {(i, k) for i, k, _ in plan.taps}
    for i, l in enumerate(plan.layers):
        conv, names = l['conv'], l['names']
        relu, pool = 'relu' in names, 'pool' in names
        tc, tr, tp = (i, 'conv') in tapped, (i, 'relu') in tapped, (i, 'pool') in tapped
        need_t = tc or not relu
        need_r = relu and (tr or (not pool and i < last) or not need_t)
        cout = conv.out_channels
        bias = conv.bias.detach() if conv.bias is not None else None
        pk, _ = _vgg_pack(conv.weight, (0, conv.in_channels), False)
        t = hip.conv_nhwc(h, pk, bias, cout, 3) if need_t else None
        r = hip.conv_nhwc(h, pk, bias, cout, 3, act=True, slope=0.0) if need_r else None
        src = r if r is not None else t
        plane = None
        if pool:
            h, plane = hip.maxpool2_nhwc(src, relu=r is None, want_plane=POOL_PLANE)
        else:
            h = src
        saved.append((src if (relu or pool) else None, r is None, plane, tuple(src.shape)))
        if tc:
            tapv[(i, 'conv')] = t
        if tr:
            tapv[(i, 'relu')] = r
        if tp:
            tapv[(i, 'pool')] = h
    return [tapv[(i, k)] for i, k, _ in plan.taps], saved


def _vgg_stack_backward(plan, b, saved, std, add_tap):
    """input gradients of the first b images back through the stack (the VGG is frozen: no weight gradients) -> d loss / d image
    [b,3,H,W], or None when no tap gave a gradient.  add_tap(g, i, kind) -> (g (None = zero) + the loss gradient of that tap,
    max |g| or None) is called for every tap position in reverse network order."""
    tapped = {(i, k) for i, k, _ in plan.taps}
    g, amax, masked = None, None, False
    for i in reversed(range(len(plan.layers))):
        l = plan.layers[i]
        conv, names = l['conv'], l['names']
        src, relu_in, plane, shape = saved[i]
        if 'pool' in names:
            g, a = add_tap(g, i, 'pool')
            amax = a if a is not None else amax
            if g is not None:
                tr = (i, 'relu') in tapped
                g, amax = hip.maxpool2_bwd_nhwc(g, None if plane is not None else src[:b], plane[:b] if plane is not None else None,
                                                relu=relu_in, mask=not tr, shape=(b,) + shape[1:])
                if tr:
                    g, _ = add_tap(g, i, 'relu')
                    g, _, _, amax = hip.act_bwd_nhwc(g, src[:b], 1, 0.0, want_bias=False, want_amax=True)
        elif 'relu' in names and not masked:
            g, a = add_tap(g, i, 'relu')
            amax = a if a is not None else amax
            if g is not None:
                g, _, _, amax = hip.act_bwd_nhwc(g, src[:b], 1, 0.0, want_bias=False, want_amax=True)
        g, a = add_tap(g, i, 'conv')
        amax = a if a is not None else amax
        if g is None:
            continue
        cin = conv.in_channels
        pk, terms = _vgg_pack(conv.weight, (0, cin), True)
        masked = False
        if i == 0:
            g4 = torch.empty(g.shape[:3] + (4,), device=g.device, dtype=torch.float32)
            hip.conv_nhwc(g, pk, None, cin, 3, out=g4[..., :cin], in_amax=amax if terms == 16 else None)
            g_x = hip.image_to_nhwc4_bwd(g4, plan.norm_img, std)
            return g_x
        prev = plan.layers[i - 1]['names']
        psrc = saved[i - 1][0]
        if terms == 16 and 'relu' in prev and 'pool' not in prev and (i - 1, 'relu') not in tapped and cin % 4 == 0:
            # the ReLU of the layer below rides on this input-gradient launch (its mask from the stored map), with max |g| of the
            # result for the next input-gradient convolution (mrefsr_conv_nhwc_bwd_f32)
            g, _, amax = hip.conv_nhwc_bwd(g, pk, cin, 3, residual=psrc[:b], residual_is_mask=True, in_amax=amax)
            masked = True
        else:
            g = hip.conv_nhwc(g, pk, None, cin, 3, in_amax=amax if terms == 16 else None)
            amax = None
    return None


def _tap_slot(plan, g, i, kind, shape, device):
    """what every add_tap of _vgg_stack_backward starts with -> (j, g, accumulate): j = the index of tap (i, kind) in plan.taps, None
    when it is none (g as it came); else g is the running gradient (accumulate) or, without one yet, a new buffer of shape(j)"""
    j = next((j for j, (ti, tk, _) in enumerate(plan.taps) if (ti, tk) == (i, kind)), None)
    if j is None or g is not None:
        return j, g, g is not None
    return j, torch.empty(shape(j), device=device, dtype=torch.float32), False


def _vgg_norm(vgg):
    """(mean, std) of the VGG's input normalisation as the kernels take them, (None, None) without one (or without a VGG)"""
    if vgg is None or not vgg.use_input_norm:
        return None, None
    return vgg.mean.contiguous(), vgg.std.contiguous()


class _VggLoss(Function):
    """(output x, gt) -> [perceptual total, style total] of PerceptualLoss with one VGG: the output and the GT run as ONE 2B batch
    through the convolution kernels (the same arithmetic for both feature sets, half the launches); the backward runs the input
    gradients of the first B images only (the VGG is frozen: no weight gradients) and returns d loss / d x."""

    @staticmethod
    def forward(ctx, x, gt, plan, mean, std):
        b = x.shape[0]
        img = torch.cat([x.detach(), gt.detach()]).contiguous()
        feats, saved = _vgg_stack_forward(plan, img, mean, std)
        if KEEP_TAPS is not None:
            KEEP_TAPS.append(feats)
        ws = [w for _, _, w in plan.taps]
        xs, ys, wts, grp = [], [], [], []
        if plan.pw > 0:
            xs += [f[:b] for f in feats]
            ys += [f[b:] for f in feats]
            wts += ws
            grp += [0] * len(feats)
        grams = []
        if plan.sw > 0:
            grams = [hip.gram_nhwc(f) for f in feats]
            xs += [g_[:b] for g_ in grams]
            ys += [g_[b:] for g_ in grams]
            wts += ws
            grp += [1] * len(feats)
        losses, totals = hip.tap_crit_loss(xs, ys, wts, grp, plan.crit if plan.pw > 0 else 'l1', (plan.pw, plan.sw))
        ctx.plan, ctx.b, ctx.saved = plan, b, saved
        ctx.save_for_backward(std, losses, *feats, *grams)
        return totals

    @staticmethod
    @once_differentiable
    def backward(ctx, g_tot):
        plan, b, saved = ctx.plan, ctx.b, ctx.saved
        st = ctx.saved_tensors
        std, losses = st[0], st[1]
        nt = len(plan.taps)
        feats, grams = st[2:2 + nt], st[2 + nt:]
        g_tot = g_tot.contiguous()

        def add_tap(g, i, kind):
            """g (None = zero) + the tap's loss gradient; -> (g, max |g|)"""
            j, g, acc = _tap_slot(plan, g, i, kind, lambda j: (b,) + tuple(feats[j].shape[1:]), g_tot.device)
            if j is None:
                return g, None
            f, w = feats[j], plan.taps[j][2]
            amax = None
            if plan.sw > 0:
                amax = hip.gram_bwd_nhwc(f[:b], grams[j][:b], grams[j][b:], g, plan.sw, w, gup=g_tot[1:2], accumulate=acc,
                                         want_amax=plan.pw <= 0)
                acc = True
            if plan.pw > 0:
                amax = hip.tap_crit_grad(f[:b], f[b:], g, w, 0, plan.crit, (plan.pw, plan.sw), gup=g_tot,
                                         norm=losses[j:j + 1] if plan.crit == 'fro' else None, accumulate=acc)
            return g, amax

        g_x = _vgg_stack_backward(plan, b, saved, std, add_tap)
        return g_x, None, None, None, None


def perceptual(vgg, x, gt, plan):
    """PerceptualLoss.forward on the training engine: -> [perceptual total, style total] (a device tensor of 2; autograd reaches x)"""
    if not (x.is_cuda and gt.is_cuda):
        raise NotImplementedError('PerceptualLoss: mrefsr_amd has no CPU path (HIP kernels only)')
    if x.dtype != torch.float32 or gt.dtype != torch.float32 or x.shape != gt.shape or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f'PerceptualLoss: two float32 [N,3,H,W] images expected, got {tuple(x.shape)} / {tuple(gt.shape)}')
    return _VggLoss.apply(x, gt, plan, *_vgg_norm(vgg))


# ---- texture loss (TextureLoss, losses.py:430-532 of the reference model's loss module) -----------------------------
TEXTURE_LAYERS = {'relu3_1': (1, 256), 'relu2_1': (2, 512), 'relu1_1': (4, 1024)}   # name -> (scale of its map, the reference's div_num)


class TextureLossPlan(VggLossPlan):
    """VggLossPlan of a TextureLoss: the taps are keys of TEXTURE_LAYERS (their weights are ignored, as in the reference); no image
    range normalisation"""

    def __init__(self, vgg_net, layer_names, loss_weight):
        bad = [n for n in layer_names if n not in TEXTURE_LAYERS]
        if bad or not layer_names:
            raise NotImplementedError(f'TextureLoss: layers {sorted(layer_names)}; only relu1_1, relu2_1 and relu3_1 have a scale and a '
                                      'divisor in the reference (it raises for any other)')
        super().__init__(vgg_net, {n: 1.0 for n in layer_names}, 'texture', 0.0, 0.0, False)
        self.names = [self.layers[i]['names'][kind] for i, kind, _ in self.taps]   # network order: the reference's summation order
        self.loss_weight = float(loss_weight)


class _VggTexture(Function):
    """(output x, per tap: coeff [B,h,w] and the Gram matrix of the weighted swapped maps [B,C,C]) -> the texture loss [1]: x through
    the VGG kernels, Fc = F * coeff, raw Gram matrices on the f32 MFMA, the Frobenius criterion of csrc/texture.hip; the backward
    adds each tap's gradient where the style term adds its own and runs the input gradients back to x."""

    @staticmethod
    def forward(ctx, x, plan, mean, std, *cg):
        import numpy as np
        nt = len(plan.taps)
        coeffs, gms = cg[:nt], cg[nt:]
        feats, saved = _vgg_stack_forward(plan, x.detach().contiguous(), mean, std)
        fcs = [hip.texture_scale_nhwc(f, c) for f, c in zip(feats, coeffs)]
        gxs = [hip.gram_raw_nhwc(fc) for fc in fcs]
        size = x.shape[-1]
        # (input_size^2 div_num)^2: a Python int in the reference, which torch rounds to fp32 for the division
        divs = [float(np.float32((size * size * TEXTURE_LAYERS[n][1]) ** 2)) for n in plan.names]
        norms, terms, total = hip.texture_crit(gxs, gms, divs, plan.loss_weight)
        ctx.plan, ctx.saved, ctx.divs = plan, saved, divs
        ctx.save_for_backward(std, norms, *fcs, *gxs, *gms, *coeffs)
        ctx.mark_non_differentiable(terms)
        return total, terms

    @staticmethod
    @once_differentiable
    def backward(ctx, g_tot, _g_terms):
        plan, saved = ctx.plan, ctx.saved
        st = ctx.saved_tensors
        std, norms = st[0], st[1]
        nt = len(plan.taps)
        fcs, gxs, gms, coeffs = (st[2 + j * nt:2 + (j + 1) * nt] for j in range(4))
        g_tot = g_tot.contiguous()
        b = fcs[0].shape[0]

        def add_tap(g, i, kind):
            j, g, acc = _tap_slot(plan, g, i, kind, lambda j: fcs[j].shape, g_tot.device)
            if j is None:
                return g, None
            scale = plan.loss_weight / 3.0 / 4.0 / ctx.divs[j]
            return g, hip.texture_gram_bwd_nhwc(fcs[j], gxs[j], gms[j], coeffs[j], norms[j:j + 1], g, scale, gup=g_tot, accumulate=acc)

        g_x = _vgg_stack_backward(plan, b, saved, std, add_tap)
        return (g_x,) + (None,) * (3 + 2 * nt)


def texture_targets(plan, maps, weights):
    """what TextureLoss needs of the swapped maps, computed once per step without autograd: per tap (network order) the coefficient map
    coeff [B,h,w] and the raw Gram matrix of maps * coeff.  maps: name -> [B,C,h,w] (read, never written); weights [B,1,gh,gw]."""
    with torch.no_grad():
        coeff = hip.texture_coeff(weights.detach().contiguous())
        coeffs, gms = [], []
        for name in plan.names:
            m = maps[name].detach().permute(0, 2, 3, 1)
            c = coeff[TEXTURE_LAYERS[name][0]]
            if tuple(m.shape[:3]) != tuple(c.shape):
                raise ValueError(f'TextureLoss: maps[{name!r}] is {tuple(maps[name].shape)}, but the weights {tuple(weights.shape)} give a '
                                 f'coefficient map of {tuple(c.shape)} at that layer')
            coeffs.append(c)
            gms.append(hip.gram_raw_nhwc(hip.texture_scale_nhwc(m.contiguous(), c)))
    return coeffs, gms


def texture(vgg, x, maps, weights, plan):
    """TextureLoss.forward on the training engine: -> (loss [1], per-layer terms [L] in network order, detached); autograd reaches x"""
    if not (x.is_cuda and weights.is_cuda and all(maps[n].is_cuda for n in plan.names)):
        raise NotImplementedError('TextureLoss: mrefsr_amd has no CPU path (HIP kernels only)')
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or weights.dtype != torch.float32 or \
            any(maps[n].dtype != torch.float32 or maps[n].dim() != 4 or maps[n].shape[0] != x.shape[0] for n in plan.names):
        raise ValueError(f'TextureLoss: a float32 [N,3,H,W] image, float32 [N,C,h,w] maps and float32 weights expected, got x {tuple(x.shape)}')
    coeffs, gms = texture_targets(plan, maps, weights)
    return _VggTexture.apply(x, plan, *_vgg_norm(vgg), *coeffs, *gms)


# ---- contextual loss (losses.ContextualLoss; Mechrez et al., ECCV 2018) ---------------------------------------------
KEEP_CX = None   # tests/ set a list: every _VggContextual forward appends, per tap (the RGB tap first), dict(jmin, imax, CX) of the device's selections


_CX_SAVED = ('xn', 'yn', 'rnorm', 'rowf', 'jmin', 'cxmax', 'imax', 'cx')   # what hip.contextual_bwd reads of hip.contextual_fwd's outputs


class ContextualLossPlan(VggLossPlan):
    """VggLossPlan of a ContextualLoss: the taps with their weights and strides, the band width, the weight of the spatial term, the
    RGB patch tap (rgb: dict(size, stride, weight) or None) and the loss weight.  vgg_net None: no VGG tap (the RGB tap alone)"""

    def __init__(self, vgg_net, layer_weights, band_width, loss_weight, norm_img, weight_sp=0.0, tap_stride=None, rgb_patch=None):
        if vgg_net is None:
            self.layers, self.taps = [], []
            self.crit, self.pw, self.sw, self.norm_img = 'contextual', 0.0, 0.0, bool(norm_img)
        else:
            super().__init__(vgg_net, layer_weights, 'contextual', 0.0, 0.0, norm_img)
        self.names = [self.layers[i]['names'][kind] for i, kind, _ in self.taps]   # network order: the summation order
        self.band_width, self.loss_weight, self.weight_sp = float(band_width), float(loss_weight), float(weight_sp)
        self.strides = [int((tap_stride or {}).get(n, 1)) for n in self.names]
        self.rgb = dict(rgb_patch) if rgb_patch else None
        if not self.taps and self.rgb is None:
            raise ValueError('ContextualLoss: no tap (neither a VGG layer nor rgb_patch)')


class _VggContextual(Function):
    """(output x, gt) -> the contextual loss [1]: output and GT as ONE 2B batch; the RGB tap, if any, on the patches of the images
    (hip.cx_patches), then the batch through the VGG kernels and per tap -- on its positions (r s, c s) when it has a stride
    (hip.cx_subsample) -- the kernels of csrc/contextual.hip (the running total is carried from tap to tap on the device, the RGB
    tap first, the VGG taps in network order); the backward adds each tap's gradient where the perceptual term adds its own (a
    strided tap's scattered by hip.cx_subsample_bwd, which hands max |g| on), runs the input gradients of the first B images back
    to x and adds the RGB tap's there (hip.cx_patches_bwd)."""

    @staticmethod
    def forward(ctx, x, gt, plan, mean, std):
        b = x.shape[0]
        img = torch.cat([x.detach(), gt.detach()]).contiguous()
        need = ctx.needs_input_grad[0]
        state = dict(run=None, total=None)
        keep = []

        def tap(name, f, w, hint):
            if f.shape[1] * f.shape[2] > hip.CX_MAX_N:
                raise NotImplementedError(f'ContextualLoss: tap {name} of {f.shape[1]} x {f.shape[2]} = {f.shape[1] * f.shape[2]} positions; '
                                          f'at most {hip.CX_MAX_N} (one N x N matrix per sample is materialised): {hint}')
            try:
                state['total'], s = hip.contextual_fwd(f[:b], f[b:], plan.band_width, w, plan.loss_weight, run=state['run'],
                                                       weight_sp=plan.weight_sp)
            except NotImplementedError as e:
                raise NotImplementedError(f'ContextualLoss: tap {name} of {f.shape[1]} x {f.shape[2]} positions: {e}') from None
            state['run'] = s['run']
            keep.append(s)

        if plan.rgb is not None:
            tap('rgb_patch', hip.cx_patches(img, plan.rgb['size'], plan.rgb['stride'], plan.norm_img), float(plan.rgb['weight']),
                'raise the stride of rgb_patch')
        feats, saved = _vgg_stack_forward(plan, img, mean, std) if plan.taps else ([], None)
        for (_, _, w), name, s, f in zip(plan.taps, plan.names, plan.strides, feats):
            tap(name, f if s == 1 else hip.cx_subsample(f, s), w,
                f"evaluate it on a sub-grid with tap_stride = {{'{name}': {max(2, s + 1)}}} or more")
        if KEEP_CX is not None:
            KEEP_CX.append([dict(jmin=s['jmin'], imax=s['imax'], CX=s['cx']) for s in keep])
        ctx.plan, ctx.b, ctx.saved, ctx.image = plan, b, saved, tuple(x.shape)
        ctx.tap_shapes = [tuple(f.shape[1:]) for f in feats]
        ctx.save_for_backward(std, *[s[k] for s in (keep if need else []) for k in _CX_SAVED])
        return state['total']

    @staticmethod
    @once_differentiable
    def backward(ctx, g_tot):
        plan, b, saved = ctx.plan, ctx.b, ctx.saved
        st = ctx.saved_tensors
        std, nk = st[0], len(_CX_SAVED)
        keep = [dict(zip(_CX_SAVED, st[1 + j * nk:1 + (j + 1) * nk])) for j in range(len(plan.taps) + (plan.rgb is not None))]
        rgb = keep.pop(0) if plan.rgb is not None else None
        g_tot = g_tot.contiguous()

        def add_tap(g, i, kind):
            j, g, acc = _tap_slot(plan, g, i, kind, lambda j: (b,) + ctx.tap_shapes[j], g_tot.device)
            if j is None:
                return g, None
            coef = plan.loss_weight * plan.taps[j][2]
            if plan.strides[j] == 1:
                return g, hip.contextual_bwd(keep[j], plan.band_width, coef, g, gup=g_tot, accumulate=acc, weight_sp=plan.weight_sp)
            gs = torch.empty_like(keep[j]['xn'])
            hip.contextual_bwd(keep[j], plan.band_width, coef, gs, gup=g_tot, want_amax=False, weight_sp=plan.weight_sp)
            return g, hip.cx_subsample_bwd(gs, g, plan.strides[j], accumulate=acc)

        g_x = _vgg_stack_backward(plan, b, saved, std, add_tap) if plan.taps else None
        if rgb is not None:
            gp = torch.empty_like(rgb['xn'])
            hip.contextual_bwd(rgb, plan.band_width, plan.loss_weight * float(plan.rgb['weight']), gp, gup=g_tot, want_amax=False,
                               weight_sp=plan.weight_sp)
            g_x = hip.cx_patches_bwd(gp, ctx.image, plan.rgb['size'], plan.rgb['stride'], scale=0.5 if plan.norm_img else 1.0, out=g_x)
        return g_x, None, None, None, None


def contextual(vgg, x, gt, plan):
    """ContextualLoss.forward on the training engine: -> the loss [1] (a device tensor; autograd reaches x).  vgg: the loss's
    VGGFeatureExtractor, None when the plan has no VGG tap"""
    if not (x.is_cuda and gt.is_cuda):
        raise NotImplementedError('ContextualLoss: mrefsr_amd has no CPU path (HIP kernels only)')
    if x.dtype != torch.float32 or gt.dtype != torch.float32 or x.shape != gt.shape or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f'ContextualLoss: two float32 [N,3,H,W] images expected, got {tuple(x.shape)} / {tuple(gt.shape)}')
    return _VggContextual.apply(x, gt, plan, *_vgg_norm(vgg))


def recording(*tensors):
    """autograd is on and one of the tensors / parameters is part of a graph"""
    return ENABLED and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def conv(mod, x1, x2, slope, prelu, pre, residual, epilogue, cin_slice, bias):
    prelu_w = None
    if prelu is not None:
        if prelu.weight.numel() != 1:
            raise NotImplementedError('nhwc.conv: per-channel PReLU')
        if hip.is_range_free():   # re-run after a PReLU slope <= 0 was met: unfused activation (its backward needs the sign of x)
            y = _Conv.apply(x1, x2, mod.weight, mod.bias if bias else None, None, pre, residual, None, epilogue, cin_slice)
            return torch.nn.functional.prelu(y, prelu.weight)
        prelu_w = prelu.weight
    return _Conv.apply(x1, x2, mod.weight, mod.bias if bias else None, prelu_w, pre, residual, slope, epilogue, cin_slice)


RESBLOCK = os.environ.get('MREFSR_TRAIN_RESBLOCK', '1') != '0'


def resblock(blk, x):
    """one residual block of a trunk as a single node, or None when it does not have that form (the caller records two convolutions)"""
    c1, c2 = blk.conv1, blk.conv2
    if not (RESBLOCK and blk.res_scale == 1 and c1.kernel_size == (3, 3) and c2.kernel_size == (3, 3) and x.shape[3] == c1.in_channels
            and c1.in_channels % 4 == 0 and c1.out_channels % 4 == 0 and c2.out_channels == c1.in_channels):
        return None
    return _ResBlock.apply(x, c1.weight, c1.bias, c2.weight, c2.bias)


RESCHAIN = os.environ.get('MREFSR_TRAIN_RESCHAIN', '1') != '0'


def reschain(blocks, x):
    """a trunk of residual blocks as a single node, or None when the blocks do not all have the plain form (3x3, one width, biases,
    res_scale 1, every parameter trained): the caller records them one by one"""
    blocks = list(blocks)
    if not (RESCHAIN and RESBLOCK and len(blocks) >= 2):
        return None
    c = x.shape[3]
    params = []
    for blk in blocks:
        for cv in (blk.conv1, blk.conv2):
            if not (cv.kernel_size == (3, 3) and cv.in_channels == c and cv.out_channels == c and c % 4 == 0 and cv.bias is not None
                    and cv.weight.requires_grad and cv.bias.requires_grad):
                return None
            params += [cv.weight, cv.bias]
        if blk.res_scale != 1:
            return None
    return _ResChain.apply(x, *params)


conv_dynagg = _ConvDynAgg.apply
dcn = _Dcn.apply
attention = _Attention.apply
modulate = _Modulate.apply
reflect_pad = _Pad.apply
crop = _Crop.apply
