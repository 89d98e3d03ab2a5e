"""torch-tensor level bindings of the C ABI (include/mrefsr_hip.h).

PyTorch is plumbing here: it owns device memory (caching allocator) and the stream; the library
gets raw device pointers + ``torch.cuda.current_stream().cuda_stream``.  No CPU path: a non-GPU
tensor raises (the reference's native ops raise NotImplementedError on CPU tensors as well,
basicsr/ops/dcn/deform_conv.py:61-62).
"""
import contextlib
import ctypes as C
import math
import weakref

import torch

from . import _lib
from .param_cache import Packed as _Packed, param_stamp   # (the one liveness rule of everything cached per parameter)
from ._lib import DcnShape


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# Optional per-kernel timing: HIP events recorded on the very stream the kernel is launched on
# (torch's current stream).  bench.py turns it on to measure the correlation kernel inside the
# timed end-to-end step; off by default (no events, no overhead).
_timing = {'on': False, 'detail': False, 'events': {}, 'work': {}}


def set_kernel_timing(on=True, detail=False):
    """on: time the correlation call; detail: also every conv_nhwc / dcn_fwd launch (hundreds of event
    pairs per step -- bench.py does that in an extra, untimed step)"""
    _timing['on'] = bool(on)
    _timing['detail'] = bool(on and detail)
    _timing['events'] = {}
    _timing['work'] = {}
    _timing['bytes'] = {}


def kernel_work():
    """{kernel: algorithmic FLOPs summed over the timed launches}"""
    return dict(_timing['work'])


def kernel_bytes():
    """{kernel: algorithmic bytes (every operand and result once) summed over the timed launches}"""
    return dict(_timing.get('bytes', {}))


def kernel_timings():
    """{kernel: [ms, ...]} -- call after torch.cuda.synchronize()."""
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in _timing['events'].items()}


class _timed:
    def __init__(self, name, flops=0.0, detail=False, nbytes=0.0):
        self.name, self.flops, self.nbytes = name, flops, nbytes
        # (an event recorded inside a hipGraph capture is a graph node, not a timestamp: elapsed_time on it is an invalid handle)
        self.active = _timing['on'] and (_timing['detail'] or not detail) and not torch.cuda.is_current_stream_capturing()

    def __enter__(self):
        if self.active:
            self.a, self.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if self.active:
            self.b.record()
            _timing['events'].setdefault(self.name, []).append((self.a, self.b))
            _timing['work'][self.name] = _timing['work'].get(self.name, 0.0) + self.flops
            _timing.setdefault('bytes', {})[self.name] = _timing.get('bytes', {}).get(self.name, 0.0) + self.nbytes


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _chk(name, *tensors, dtype=torch.float32):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise NotImplementedError(f'{name}: tensor on {t.device}; mrefsr_amd has no CPU path (HIP kernels only)')
        if t.dtype != dtype:
            raise TypeError(f'{name}: expected {dtype}, got {t.dtype}')
        if not t.is_contiguous():
            raise ValueError(f'{name}: tensor must be contiguous')


def _c(t):
    return t if t is None or t.is_contiguous() else t.contiguous()


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


# ------------------------------------------------------------------ cached device memory
# Device memory that outlives a wrapper call (scratch, zeroed ticket / level-set words, zero-filled accumulator chunks) is cached
# per (device, stream, side of a hipGraph capture boundary[, extra key]) in instances of ONE class, and the capture bookkeeping
# (release_capture_workspaces, capture_refs, capture_ptrs) runs over all of them: a new cache is an instance, nothing else.
def _stream_side():
    """(handle of torch's current stream, whether it is capturing): the caches and capture_epoch() read both here, nowhere else"""
    # (the raw handle, 0.7 us for the pair: torch.cuda.current_stream() builds a Stream object per call, 2.7 us, and capture_epoch()
    #  is asked once per packed weight, ~340 times per training step)
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()), torch.cuda.is_current_stream_capturing()


_caches = []


class _StreamCache:
    """entries per (device index, stream handle, capturing, extra).  Per stream: launches on ONE stream are ordered, two eager
    streams sharing a buffer would overwrite each other's contents.  Per side: a buffer handed out under a capture comes from the
    graph's pool and its address is baked into the graph -- the graph's owner keeps it (capture_refs), it is dropped with the
    graph (release_capture_workspaces), and nothing an eager call does replaces it.  tensor: entry -> its buffer"""

    def __init__(self, tensor=lambda e: e):
        self.entries, self.tensor = {}, tensor
        _caches.append(self)

    def key(self, device, extra=None):
        return (device.index, *_stream_side(), extra)

    def captured(self):
        return [k for k in self.entries if k[2]]


_scratch_bufs, _zeroed, _zero_chunks = _StreamCache(), _StreamCache(), _StreamCache(tensor=lambda ch: ch[0])


def _scratch(device, nbytes):
    """>= nbytes of uint8 scratch (256-byte aligned; at least 1 MiB, so that warm-up does not reallocate at every slightly larger
    request), one growing buffer per cache key.  THE RULE: its contents are dead once the launches of the wrapper call that asked
    for it are enqueued -- launches on a stream are ordered, and the next wrapper call on that stream may take the same bytes.
    So a wrapper asks ONCE per call (two regions at once: one request, sliced at 256-byte alignment), reads nothing a previous
    call left here, and passes the library the byte count it asked for, not the buffer's size"""
    key = _scratch_bufs.key(device)
    buf = _scratch_bufs.entries.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _scratch_bufs.entries[key] = torch.empty(max(nbytes, 1 << 20), device=device, dtype=torch.uint8)
    return buf


def _zeroed_words(device, name, n):
    """n int32 words zeroed once that every launch using them leaves zero again (tickets, level sets), per cache key and (name, n)"""
    key = _zeroed.key(device, (name, n))
    t = _zeroed.entries.get(key)
    if t is None:
        t = _zeroed.entries[key] = torch.zeros(n, device=device, dtype=torch.int32)
    return t


def release_capture_workspaces():
    """drop every cached buffer that was handed out under a capture (call when the graphs that used them are destroyed)"""
    for c in _caches:
        for k in c.captured():
            del c.entries[k]


def capture_refs():
    """the cached buffers whose addresses a hipGraph captured now may have baked in: whoever owns the graph keeps this list as
    long as the graph lives"""
    # (only the buffers that were handed out UNDER a capture: an eager regrowth of some other stream's scratch -- validation at
    #  another size, the correlation call's scratch -- does not move anything a graph baked in, and must not force a recapture)
    return [c.tensor(c.entries[k]) for c in _caches for k in c.captured()]


def capture_ptrs():
    """addresses of the cached buffers of capture_refs(): a graph owner compares them before a replay (a regrown buffer has moved)"""
    return tuple(t.data_ptr() for t in capture_refs())


_cap_state = [False, 0]


def _epoch(cap):
    if cap != _cap_state[0]:
        _cap_state[0] = cap
        _cap_state[1] += 1
    return cap, _cap_state[1]


def capture_epoch():
    """(capturing, epoch): the epoch moves every time this is called on the other side of a hipGraph capture boundary than
    the call before -- device state prepared on one side (zero-filled accumulators, packed weight copies) is not replayed with
    a graph captured on the other, so its users key it by this epoch"""
    return _epoch(_stream_side()[1])


_ZCHUNK = 1 << 18
_ZALIGN = 128         # floats: slices start on 512-byte boundaries like allocations of their own (float atomics into a slice at
                      # 16-byte granularity ran 17 % slower: act_bwd_nhwc 5.66 -> 4.87 ms per training step)


def zeros_f32(device, n):
    """n zero float32 (512-byte aligned) carved from a chunk that ONE fill launch zeroed: the accumulators of act_bwd_nhwc (bias
    gradient, PReLU slope gradient, max |g|: ~70 floats, 174 times per training step) each had a fill launch of their own.  A
    slice is handed out once and never re-zeroed, so it may be kept (autograd adopts the bias gradient as ``.grad``); the chunk
    lives as long as any of its slices.  Chunks are per stream and per side of a capture boundary (the fill that zeroes a chunk
    has to be part of the graph whose kernels accumulate into it)."""
    key = _zero_chunks.key(device)
    _, epoch = _epoch(key[2])
    n4 = (n + _ZALIGN - 1) // _ZALIGN * _ZALIGN
    ch = _zero_chunks.entries.get(key)
    if ch is None or ch[2] != epoch or ch[1] + n4 > ch[0].numel():
        ch = _zero_chunks.entries[key] = [torch.zeros(max(_ZCHUNK, n4), device=device, dtype=torch.float32), 0, epoch]
    out = ch[0][ch[1]:ch[1] + n]
    ch[1] += n4
    return out

# ------------------------------------------------------------------ deterministic mode
# net_g's backward adds three kinds of per-channel sums over blocks with float atomics (bias gradients and the PReLU slope gradient
# in act_bwd_nhwc, conv_offset_mask's bias gradient in dynagg_prep_bwd_nhwc, the per-cout sums in the epilogue of conv_nhwc_bwd):
# the order of the blocks is the hardware's.  With the switch on, those three calls take the library's *_det_f32 entry points:
# one workspace row per block, added in block order by the block that finishes last -- the same launches, the same element-wise
# bits, sums that two runs agree on bit for bit.  Off (the default), nothing changes.
_deterministic = [None]   # None: follow torch.are_deterministic_algorithms_enabled()


def set_deterministic(mode):
    """True / False: fixed-order gradient reductions on / off; None (the default): as torch.use_deterministic_algorithms says"""
    if mode is not None and not isinstance(mode, bool):
        raise TypeError(f'set_deterministic: True, False or None expected, got {mode!r}')
    _deterministic[0] = mode


def is_deterministic():
    mode = _deterministic[0]
    return torch.are_deterministic_algorithms_enabled() if mode is None else mode


class deterministic:
    """``with hip.deterministic():`` -- the switch on (or ``deterministic(False)``: off) inside the block, what it was behind it.
    The switch is one per process, not per thread: autograd runs the backward on a thread of its own."""

    def __init__(self, mode=True):
        if mode is not None and not isinstance(mode, bool):
            raise TypeError(f'deterministic: True, False or None expected, got {mode!r}')
        self.mode = mode

    def __enter__(self):
        self.prev = _deterministic[0]
        _deterministic[0] = self.mode
        return self

    def __exit__(self, *exc):
        _deterministic[0] = self.prev


def nondeterministic_alert(what):
    """for an operation that has no fixed-order form (the float-atomic scatter of the DCN input gradient): with the switch on raise
    like torch does -- or only warn when torch.use_deterministic_algorithms(True, warn_only=True) says so"""
    if not is_deterministic():
        return
    msg = (f'{what} does not have a deterministic implementation, but you set mrefsr_amd.hip.set_deterministic(True) / '
           "'torch.use_deterministic_algorithms(True)' (or train.deterministic: true). You can turn the mode off for this operation "
           'with `with mrefsr_amd.hip.deterministic(False):`, or ask for warnings only with '
           "'torch.use_deterministic_algorithms(True, warn_only=True)'.")
    if torch.is_deterministic_algorithms_warn_only_enabled():
        import warnings
        warnings.warn(msg)
    else:
        raise RuntimeError(msg)


def _det_scratch(device, nbytes):
    """(partials scratch, ticket word) of one deterministic reduction launch: every launch leaves the ticket zero again"""
    return _scratch(device, max(int(nbytes), 4)), _zeroed_words(device, 'ticket', 1)


# ------------------------------------------------------------------ correlation path
def padded_channels(c):
    r = _lib.load().mrefsr_corr_padded_channels(int(c))
    if r < 0:
        raise _lib.MrefsrHipError(_lib.load().mrefsr_last_error().decode())
    return r


def pixnorm(x, normalize=True, want_bf16_split=False, nhwc=False, split='bf16', want_err=False):
    """x [N,C,h,w] (or [N,h,w,C] with nhwc=True) -> (y [N,h*w,Cp] split layout, n2 [N,h,w][, pre-filter operand][, d2]).
    want_bf16_split: also return the pre-filter operand -- split='bf16': [N,h*w,2,Cp] bf16 hi|lo;
    split='fp16': [N,h*w,Cp] float16 (the single-plane pre-filter, Cp = 256 only).
    want_err: also d2 [N,h,w], the squared norm of each pixel vector's fp16 rounding error (prefilter_window)."""
    x16 = x.dtype == torch.bfloat16
    if x16 and not nhwc:
        raise TypeError('pixnorm: bf16 feature maps are accepted channels-last only')
    _chk('pixnorm', x, dtype=x.dtype if x16 else torch.float32)
    if nhwc:
        n, h, w, c = x.shape
    else:
        n, c, h, w = x.shape
    cp = padded_channels(c)
    y = torch.empty((n, h * w, cp), device=x.device, dtype=torch.float32)
    n2 = torch.empty((n, h, w), device=x.device, dtype=torch.float32)
    ybf = None
    if want_bf16_split:
        # + (6 image rows + 16 pixels) of slack: the pre-filter's LDS-DMA staging reads edge tiles
        # (8 rows x 16 pixels from an origin <= (h-3, w-3)) unclamped: include/mrefsr_hip.h,
        # mrefsr_corr_top1_prefilter_f32
        if split == 'fp16':
            flat = torch.empty(n * h * w * cp + (6 * w + 16) * cp, device=x.device, dtype=torch.float16)
            ybf = flat[:n * h * w * cp].view(n, h * w, cp)
        else:
            flat = torch.empty(n * h * w * 2 * cp + (6 * w + 16) * 2 * cp, device=x.device, dtype=torch.bfloat16)
            ybf = flat[:n * h * w * 2 * cp].view(n, h * w, 2, cp)
    d2 = torch.empty((n, h, w), device=x.device, dtype=torch.float32) if want_err else None
    _lib.call('mrefsr_pixnorm_f32', _p(x), _p(y), _p(n2), _p(ybf), n, c, h * w, 1 if normalize else 0, (2 if x16 else 1) if nhwc else 0,
              1 if split == 'fp16' else 0, _p(d2), _stream())
    out = (y, n2, ybf) if want_bf16_split else (y, n2)
    return out + (d2,) if want_err else out


def prefilter_window(nrm_in, inv_ref, d2_in, d2_ref):
    """Per-query window of the fp16 pre-filter (include/mrefsr_hip.h, mrefsr_corr_top1_prefilter_f32): twice a proven
    bound on |approximate - canonical score|.  nrm_in [n_in,P'], inv_ref [n_pair,P'] from patch_norm of the n2 maps,
    d2_* from pixnorm(want_err=True).  Returns tau [n_pair, P'] (pair p uses input p % n_in)."""
    d_in, _ = patch_norm(d2_in)                      # sqrt(3x3 sum of d2) + 1e-5  >=  D
    d_ref, _ = patch_norm(d2_ref)
    n_in, n_pair = nrm_in.shape[0], inv_ref.shape[0]
    rho = (d_ref * inv_ref).flatten(1).amax(1)       # [n_pair]: largest relative rounding error of a reference patch
    rho = torch.nan_to_num(rho, nan=1.0, posinf=1.0).view(n_pair // n_in, n_in, 1, 1)
    dq, nq = d_in.unsqueeze(0), nrm_in.unsqueeze(0)  # [1,n_in,h-2,w-2]
    tau = 2.02 * (dq + (nq + 3.0 * dq) * rho) + 2.0e-4 * nq
    return tau.reshape(n_pair, *nrm_in.shape[1:]).contiguous()


def patch_norm(n2):
    """n2 [N,h,w] -> (norm+1e-5 [N,h-2,w-2], 1/(norm+1e-5))."""
    _chk('patch_norm', n2)
    n, h, w = n2.shape
    ne = torch.empty((n, h - 2, w - 2), device=n2.device, dtype=torch.float32)
    inv = torch.empty_like(ne)
    _lib.call('mrefsr_patch_norm_f32', _p(n2), _p(ne), _p(inv), n, h, w, _stream())
    return ne, inv


def corr_top1(y_in, y_ref, inv_ref, nrm_in, h, w, want_val=True, ybf_in=None, ybf_ref=None, tau=None):
    """y_in [n_in,h*w,Cp], y_ref [n_pair,h*w,Cp] -> (max_idx int64 [n_pair,h-2,w-2], max_val|None).
    With the bf16 / fp16 pre-filter operands given, the pre-filter + exact re-scoring path runs (same bits out);
    tau (fp16 operands only): the per-query window from prefilter_window(), else the worst-case window."""
    _chk('corr_top1', y_in, y_ref, inv_ref, nrm_in)
    n_in, hw, cp = y_in.shape
    n_pair = y_ref.shape[0]
    if hw != h * w or y_ref.shape[1] != hw or y_ref.shape[2] != cp:
        raise ValueError('corr_top1: input / reference feature sizes differ '
                         '(the path assumes equal sizes: corres_generation_arch.py:33-35)')
    if n_pair % n_in:
        raise ValueError(f'corr_top1: n_pair={n_pair} not a multiple of n_in={n_in}')
    idx = torch.empty((n_pair, h - 2, w - 2), device=y_in.device, dtype=torch.int64)
    val = torch.empty((n_pair, h - 2, w - 2), device=y_in.device, dtype=torch.float32) if want_val else None
    if ybf_in is not None and ybf_ref is not None:
        fmt = 1 if ybf_in.dtype == torch.float16 else 0
        _chk('corr_top1', ybf_in, ybf_ref, dtype=torch.float16 if fmt else torch.bfloat16)
        if tau is not None:
            _chk('corr_top1', tau)
            if not fmt or tuple(tau.shape) != (n_pair, h - 2, w - 2):
                raise ValueError('corr_top1: tau is [n_pair,h-2,w-2] and belongs to the fp16 pre-filter operand')
        need = _lib.load().mrefsr_corr_workspace_bytes(n_pair, h, w)
        ws = _scratch(y_in.device, need)   # (~400 MB at the benchmark size, used and dropped within this call; a fresh torch.empty
                                           #  per call held a second copy of it alive in the allocator across the whole pass)
        # diagnostic hook (tools/corr_diag.py): the bytes last only until the next scratch user on this stream -- read them at once
        _timing['last_corr_ws'] = (ws, n_pair, (h - 2) * (w - 2)) if _timing.get('keep_ws') else None
        with _timed('corr_top1'):
            _lib.call('mrefsr_corr_top1_prefilter_f32', _p(y_in), _p(y_ref), _p(ybf_in), _p(ybf_ref), _p(inv_ref),
                      _p(nrm_in), _p(idx), _p(val), _p(ws), C.c_int64(need), n_in, n_pair, cp, h, w, fmt, _p(tau), _stream())
        return idx, val
    with _timed('corr_top1'):
        _lib.call('mrefsr_corr_top1_f32', _p(y_in), _p(y_ref), _p(inv_ref), _p(nrm_in), _p(idx), _p(val), n_in, n_pair,
                  cp, h, w, _stream())
    return idx, val


def feature_match_index_generic(feat_in, feat_ref, patch_size, input_stride, ref_stride, is_norm, norm_input):
    """feat_in (C,h,w), feat_ref (C,hr,wr) -> (max_idx int64 (nqy,nqx), max_val fp32): any patch size / strides / sizes"""
    _chk('feature_match_index', feat_in, feat_ref)
    c, h, w = feat_in.shape
    cr, hr, wr = feat_ref.shape
    if c != cr:
        raise ValueError('feature_match_index: channel counts differ')
    if min(h, w, hr, wr) < patch_size:
        raise ValueError('feature_match_index: a map is smaller than the patch')
    nqy, nqx = (h - patch_size) // input_stride + 1, (w - patch_size) // input_stride + 1
    idx = torch.empty((nqy, nqx), device=feat_in.device, dtype=torch.int64)
    val = torch.empty((nqy, nqx), device=feat_in.device, dtype=torch.float32)
    need = _lib.load().mrefsr_feature_match_index_workspace_bytes(h, w, hr, wr)
    ws = torch.empty(need, device=feat_in.device, dtype=torch.uint8)
    _lib.call('mrefsr_feature_match_index_f32', _p(feat_in), _p(feat_ref), c, h, w, hr, wr, int(patch_size), int(input_stride), int(ref_stride),
              1 if is_norm else 0, 1 if norm_input else 0, _p(idx), _p(val), _p(ws), C.c_int64(need), _stream())
    return idx, val


def offsets_from_idx(idx, h, w, scales=(1, 2, 4)):
    """idx int64 [N,h-2,w-2] -> dict scale -> [N,9,s*h,s*w,2] fp32 ([x,y])."""
    _chk('offsets_from_idx', idx, dtype=torch.int64)
    n = idx.shape[0]
    outs = {s: torch.empty((n, 9, s * h, s * w, 2), device=idx.device, dtype=torch.float32) for s in scales}
    _lib.call('mrefsr_offsets_from_idx_f32', _p(idx), _p(outs.get(1)), _p(outs.get(2)), _p(outs.get(4)), n, h, w,
              _stream())
    return outs


# ------------------------------------------------------------------ DynAgg glue
def dynagg_prep(om, pre, dg, abs_sum=None, om_bias=None, om_nhwc=False):
    """om [B,27dg,H,W] (or [B,H,W,27dg] with om_nhwc) -> planar (offset [B,18dg,H,W], mask [B,9dg,H,W])"""
    _chk('dynagg_prep', om, pre, om_bias)
    if om_nhwc:
        b, h, w, ch = om.shape
    else:
        b, ch, h, w = om.shape
    if ch != 27 * dg or tuple(pre.shape) != (b, 9, h, w, 2):
        raise ValueError(f'dynagg_prep: om {tuple(om.shape)} / pre {tuple(pre.shape)} inconsistent with dg={dg}')
    offset = torch.empty((b, 18 * dg, h, w), device=om.device, dtype=torch.float32)
    mask = torch.empty((b, 9 * dg, h, w), device=om.device, dtype=torch.float32)
    if abs_sum is not None:
        _chk('dynagg_prep', abs_sum, dtype=torch.float64)
    _lib.call('mrefsr_dynagg_prep_f32', _p(om), _p(om_bias), _p(pre), _p(offset), _p(mask), _p(abs_sum), b, dg, h, w,
              1 if om_nhwc else 0, _stream())
    return offset, mask


def dynagg_prep_bwd(g_offset, g_mask, mask, dg):
    _chk('dynagg_prep_bwd', g_offset, g_mask, mask)
    b, _, h, w = mask.shape
    g_om = torch.empty((b, 27 * dg, h, w), device=mask.device, dtype=torch.float32)
    _lib.call('mrefsr_dynagg_prep_bwd_f32', _p(g_offset), _p(g_mask), _p(mask), _p(g_om), b, dg, h, w, _stream())
    return g_om


def dynagg_prep_bwd_nhwc(g_offset, g_mask, mask, dg, want_bias=True):
    """dynagg_prep_bwd with the result channels-last [B,H,W,27dg] and, from the same pass, (bias gradient [27dg] | None, max |g_om| [1])"""
    _chk('dynagg_prep_bwd_nhwc', g_offset, g_mask, mask)
    b, _, h, w = mask.shape
    nc = 27 * dg
    g_om = torch.empty((b, h, w, nc), device=mask.device, dtype=torch.float32)
    z = zeros_f32(mask.device, nc + 1)
    if want_bias and is_deterministic():   # the bias gradient added in block order (bitwise reproducible)
        need = _lib.load().mrefsr_dynagg_prep_bwd_det_workspace_bytes(b, dg, h, w)
        ws, ticket = _det_scratch(mask.device, need)
        _lib.call('mrefsr_dynagg_prep_bwd_nhwc_det_f32', _p(g_offset), _p(g_mask), _p(mask), _p(g_om), _p(z[:nc]), _p(z[nc:]), b, dg, h, w,
                  _p(ws), C.c_int64(need), _p(ticket), _stream())
        return g_om, z[:nc], z[nc:]
    _lib.call('mrefsr_dynagg_prep_bwd_nhwc_f32', _p(g_offset), _p(g_mask), _p(mask), _p(g_om), _p(z[:nc]) if want_bias else None, _p(z[nc:]), b, dg, h, w,
              _stream())
    return g_om, (z[:nc] if want_bias else None), z[nc:]


# ------------------------------------------------------------------ DCN
def dcn_shape(x, weight, stride, padding, dilation, groups, dg):
    def pair(v):
        return (v, v) if isinstance(v, int) else tuple(v)
    (sh, sw), (ph, pw), (dh, dw) = pair(stride), pair(padding), pair(dilation)
    b, c, h, w = x.shape
    co, cig, kh, kw = weight.shape
    if cig * groups != c:
        raise RuntimeError(f"Input shape and kernel channels won't match: ({c} vs {cig * groups}).")
    s = DcnShape(b, c, h, w, co, kh, kw, sh, sw, ph, pw, dh, dw, groups, dg)
    ho = (h + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    wo = (w + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    return s, ho, wo


def dcn_mfma_eligible(c, co, dg, k=3):
    """True when mrefsr_dcn_fwd_f32 runs its fused gather+MFMA kernel for a stride-1 'same' k x k DCN"""
    s = DcnShape(1, c, 8, 8, co, k, k, 1, 1, k // 2, k // 2, 1, 1, 1, dg)
    return _lib.load().mrefsr_dcn_fwd_workspace_bytes(C.byref(s)) > 0


def dcn_fwd(x, offset, mask, weight, bias, stride, padding, dilation, groups, dg, act_slope=1.0, nhwc_gather=True,
            channels_last=False, bf16_arith=False, range_free=False, out_amax=None):
    """x NCHW.  For MFMA-eligible shapes the input is re-laid out to NHWC once (one HBM pass) so the
    deformable gather reads 16-byte channel vectors instead of scalar corners (nhwc_gather=False
    keeps the NCHW gather).  channels_last=True: x is given [B,H,W,C] and the result is [B,Ho,Wo,Co]
    (the inference path; MFMA-eligible shapes only); offset / mask are planar either way."""
    if x.dtype in (torch.float16, torch.float64):   # the reference's other dtypes: portable kernels (mrefsr_dcn_fwd)
        if channels_last:
            raise TypeError('dcn_fwd: channels_last is an fp32 / bf16 fast path')
        _chk('dcn_fwd', x, offset, mask, weight, bias, dtype=x.dtype)
        s, ho, wo = dcn_shape(x, weight, stride, padding, dilation, groups, dg)
        kk = s.kh * s.kw
        if tuple(offset.shape) != (s.B, 2 * dg * kk, ho, wo) or (mask is not None and tuple(mask.shape) != (s.B, dg * kk, ho, wo)):
            raise RuntimeError(f'dcn_fwd: offset {tuple(offset.shape)} / mask shape mismatch')
        out = torch.empty((s.B, s.Co, ho, wo), device=x.device, dtype=x.dtype)
        _lib.call('mrefsr_dcn_fwd', _p(x), _p(offset), _p(mask), _p(weight), _p(bias), _p(out), C.byref(s), C.c_float(act_slope), _DT[x.dtype],
                  _stream())
        return out
    io16 = channels_last and x.dtype == torch.bfloat16
    _chk('dcn_fwd', x, dtype=x.dtype if io16 else torch.float32)
    _chk('dcn_fwd', offset, mask, weight, bias)
    range_free = range_free or _range_free[0]
    if io16 and not bf16_arith:
        raise TypeError('dcn_fwd: bf16 tensors go with bf16_arith=True')
    if channels_last:
        s, ho, wo = dcn_shape(x.permute(0, 3, 1, 2), weight, stride, padding, dilation, groups, dg)
        need = _lib.load().mrefsr_dcn_fwd_workspace_bytes(C.byref(s))
        if need <= 0:
            raise _lib.MrefsrHipError('dcn_fwd(channels_last): shape is not eligible for the fused MFMA kernel')
        if tuple(offset.shape) != (s.B, 2 * dg * 9, ho, wo) or (mask is not None and tuple(mask.shape) != (s.B, dg * 9, ho, wo)):
            raise RuntimeError(f'dcn_fwd: offset {tuple(offset.shape)} / mask shape mismatch')
        out = torch.empty((s.B, ho, wo, s.Co), device=x.device, dtype=x.dtype)
        with _timed('dcn_fwd', 2.0 * s.B * ho * wo * s.C * s.Co * 9, detail=True):
            _lib.call('mrefsr_dcn_fwd_amax_f32', _p(x), _p(offset), _p(mask), _p(weight), _p(bias), _p(out), C.byref(s),
                      C.c_float(act_slope), (23 if io16 else 7) if bf16_arith else (11 if range_free else 3), _p(_scratch(x.device, need)), C.c_int64(need),
                      _p(_range_flag(x.device)), _p(out_amax), _stream())
        return out
    s, ho, wo = dcn_shape(x, weight, stride, padding, dilation, groups, dg)
    kk = s.kh * s.kw
    if tuple(offset.shape) != (s.B, 2 * dg * kk, ho, wo):
        raise RuntimeError(f'dcn_fwd: offset shape {tuple(offset.shape)} != {(s.B, 2 * dg * kk, ho, wo)}')
    if mask is not None and tuple(mask.shape) != (s.B, dg * kk, ho, wo):
        raise RuntimeError(f'dcn_fwd: mask shape {tuple(mask.shape)} != {(s.B, dg * kk, ho, wo)}')
    out = torch.empty((s.B, s.Co, ho, wo), device=x.device, dtype=torch.float32)
    need = _lib.load().mrefsr_dcn_fwd_workspace_bytes(C.byref(s))
    ws = _scratch(x.device, need) if need > 0 else None
    nhwc = (9 if range_free else 1) if (need > 0 and nhwc_gather) else 0
    xin = x.permute(0, 2, 3, 1).contiguous() if nhwc else x
    _lib.call('mrefsr_dcn_fwd_f32', _p(xin), _p(offset), _p(mask), _p(weight), _p(bias), _p(out), C.byref(s),
              C.c_float(act_slope), nhwc, _p(ws), C.c_int64(need), _p(_range_flag(x.device)) if nhwc else None, _stream())
    return out


def dcn_im2col(x, offset, mask, weight_shape, stride, padding, dilation, groups, dg):
    _chk('dcn_im2col', x, offset, mask, dtype=x.dtype if x.dtype in (torch.float16, torch.float64) else torch.float32)
    fake_w = torch.empty(weight_shape, device='meta')
    s, ho, wo = dcn_shape(x, fake_w, stride, padding, dilation, groups, dg)
    col = torch.empty((s.B, s.C * s.kh * s.kw, ho * wo), device=x.device, dtype=x.dtype)
    if x.dtype == torch.float32:
        _lib.call('mrefsr_dcn_im2col_f32', _p(x), _p(offset), _p(mask), _p(col), C.byref(s), _stream())
    else:
        _lib.call('mrefsr_dcn_im2col', _p(x), _p(offset), _p(mask), _p(col), C.byref(s), _DT[x.dtype], _stream())
    return col


def dcn_col2im(grad_col, x, offset, mask, weight_shape, stride, padding, dilation, groups, dg, need_grad_x=True):
    if need_grad_x:
        nondeterministic_alert('dcn_col2im (the float-atomic scatter of the deformable convolution\'s input gradient)')
    if x.dtype == torch.float16:   # gradients of an f16 call are accumulated in f32 (atomics), then rounded
        gx, goff, gmask = dcn_col2im(grad_col.float(), x.float(), offset.float(), None if mask is None else mask.float(), weight_shape, stride,
                                     padding, dilation, groups, dg, need_grad_x)
        return (None if gx is None else gx.half()), goff.half(), (None if gmask is None else gmask.half())
    _chk('dcn_col2im', grad_col, x, offset, mask, dtype=x.dtype if x.dtype == torch.float64 else torch.float32)
    fake_w = torch.empty(weight_shape, device='meta')
    s, _, _ = dcn_shape(x, fake_w, stride, padding, dilation, groups, dg)
    gx = torch.zeros_like(x) if need_grad_x else None
    goff = torch.empty_like(offset)
    gmask = torch.empty_like(mask) if mask is not None else None
    if x.dtype == torch.float64:
        _lib.call('mrefsr_dcn_col2im', _p(grad_col), _p(x), _p(offset), _p(mask), _p(gx), _p(goff), _p(gmask), C.byref(s), _DT[x.dtype], _stream())
    else:
        _lib.call('mrefsr_dcn_col2im_f32', _p(grad_col), _p(x), _p(offset), _p(mask), _p(gx), _p(goff), _p(gmask),
                  C.byref(s), _stream())
    return gx, goff, gmask


def _dcn_bwd_shapes(name, g_out, x, offset, mask, dg):
    """the backward kernels index offset / mask / g_out from x's B, H, W and dg: a mismatch would read out of bounds"""
    b, h, w, c = x.shape
    if g_out.dim() != 4 or tuple(g_out.shape[:3]) != (b, h, w):
        raise ValueError(f'{name}: g_out {tuple(g_out.shape)} does not match x {tuple(x.shape)} (channels-last, stride 1)')
    if dg < 1 or c % dg or tuple(offset.shape) != (b, 18 * dg, h, w):
        raise ValueError(f'{name}: offset {tuple(offset.shape)} != {(b, 18 * dg, h, w)} for x {tuple(x.shape)}, deformable groups {dg}')
    if mask is not None and tuple(mask.shape) != (b, 9 * dg, h, w):
        raise ValueError(f'{name}: mask {tuple(mask.shape)} != {(b, 9 * dg, h, w)}')


def dcn_bwd_data(g_out, x, offset, mask, packed_wT, dg, g_amax=None, need_grad_x=True):
    """Fused backward of DCNv2 (3x3, stride 1, pad 1) w.r.t. offset, mask and input (mrefsr_dcn_bwd_data_f32): g_out [B,H,W,Co] and
    x [B,H,W,C] channels-last, offset / mask planar; packed_wT = conv_pack_view(weight, terms=16, dgrad='T', wscale=...);
    g_amax: device float max |g_out| (None: no scaling).  -> (grad_x planar [B,C,H,W] | None, grad_offset, grad_mask | None)"""
    if need_grad_x:
        nondeterministic_alert('dcn_bwd_data (the float-atomic scatter of the deformable convolution\'s input gradient)')
    _chk('dcn_bwd_data', g_out, x, offset, mask, g_amax)
    b, h, w, c = x.shape
    co = g_out.shape[3]
    _dcn_bwd_shapes('dcn_bwd_data', g_out, x, offset, mask, dg)
    if packed_wT.terms != 16:
        raise ValueError('dcn_bwd_data: the transposed weights packed with terms=16 expected')
    s = _lib.DcnShape(b, c, h, w, co, 3, 3, 1, 1, 1, 1, 1, 1, 1, dg)
    gx = torch.zeros((b, c, h, w), device=x.device, dtype=torch.float32) if need_grad_x else None
    goff = torch.empty_like(offset)
    gmask = torch.empty_like(mask) if mask is not None else None
    _lib.call('mrefsr_dcn_bwd_data_f32', _p(g_out), _p(x), _p(offset), _p(mask), _p(packed_wT.data), C.c_float(packed_wT.wscale), _p(g_amax),
              _p(gx), _p(goff), _p(gmask), C.byref(s), _stream())
    return gx, goff, gmask


def conv_wgrad1x1(x, g, cin, cout, g_amax):
    """weight gradient [cout, cin, 1, 1] of a 1x1 convolution from channels-last storage (x [..., >= cin], g [..., >= cout], both
    pixel-contiguous views): mrefsr_conv_wgrad1x1_f32"""
    _chk('conv_wgrad1x1', g_amax)
    ld_x, ld_g = _nhwc_ld('x', x), _nhwc_ld('g', g)
    pixels = x.shape[0] * x.shape[1] * x.shape[2]
    nbytes = _lib.load().mrefsr_conv_wgrad1x1_workspace_bytes(pixels, cout, cin)
    ws = _scratch(x.device, nbytes)
    gw = torch.empty((cout, cin, 1, 1), device=x.device, dtype=torch.float32)
    _lib.call('mrefsr_conv_wgrad1x1_f32', _p(g), _p(x), _p(g_amax), _p(gw), _p(ws), nbytes, pixels, cout, ld_g, cin, ld_x,
              _p(_range_flag(x.device)), _stream())
    return gw


def dcn_bwd_weight(g_out, x, offset, mask, cout, dg, g_amax=None):
    """d weight [Co,C,3,3] of DCNv2 (3x3, stride 1, pad 1) with the columns re-gathered inside the GEMM (mrefsr_dcn_bwd_weight_f32);
    tensors as dcn_bwd_data"""
    _chk('dcn_bwd_weight', g_out, x, offset, mask, g_amax)
    b, h, w, c = x.shape
    _dcn_bwd_shapes('dcn_bwd_weight', g_out, x, offset, mask, dg)
    s = _lib.DcnShape(b, c, h, w, cout, 3, 3, 1, 1, 1, 1, 1, 1, 1, dg)
    nbytes = _lib.load().mrefsr_dcn_bwd_weight_workspace_bytes(C.byref(s))
    ws = _scratch(x.device, nbytes)
    gw = torch.empty((cout, c, 3, 3), device=x.device, dtype=torch.float32)
    _lib.call('mrefsr_dcn_bwd_weight_f32', _p(g_out), _p(x), _p(offset), _p(mask), _p(g_amax), _p(gw), _p(ws), nbytes, C.byref(s),
              _p(_range_flag(x.device)), _stream())
    return gw


# ------------------------------------------------------------------ attention core
def mrattn_fwd(q, emb, ass, t, want_prob=True, t_major=False):
    """q [N,c,H,W], emb [N*T,c,H,W], ass [N*T,c2,H,W] -> (out [N,c2,H,W], prob [N,T,H,W]|None)."""
    _chk('mrattn_fwd', q, emb, ass)
    n, c, h, w = q.shape
    c2 = ass.shape[1]
    if emb.shape[0] != n * t or ass.shape[0] != n * t or emb.shape[1] != c:
        raise ValueError('mrattn_fwd: inconsistent shapes')
    out = torch.empty((n, c2, h, w), device=q.device, dtype=torch.float32)
    prob = torch.empty((n, t, h, w), device=q.device, dtype=torch.float32) if want_prob else None
    _lib.call('mrefsr_mrattn_fwd_f32', _p(q), _p(emb), _p(ass), _p(out), _p(prob), n, t, c, c2, h * w, 1 if t_major else 0, _stream())
    return out, prob


def mrattn_fwd_nhwc(q, emb, ass, t, q_scale=None):
    """q [N,H,W,c], emb [t*N,H,W,c], ass [t*N,H,W,2c] (t-major) -> out [N,H,W,2c]; q_scale (fp32 tensors): the attention of
    q * q_scale, the products formed in the kernel as the separate pass would have rounded them"""
    b16 = q.dtype == torch.bfloat16
    if q_scale is not None and b16:
        raise TypeError('mrattn_fwd_nhwc: q_scale goes with fp32 tensors')
    _chk('mrattn_fwd_nhwc', q, emb, ass, dtype=q.dtype if b16 else torch.float32)
    n, h, w, c = q.shape
    if tuple(emb.shape) != (n * t, h, w, c) or tuple(ass.shape) != (n * t, h, w, 2 * c):
        raise ValueError('mrattn_fwd_nhwc: inconsistent shapes')
    out = torch.empty((n, h, w, 2 * c), device=q.device, dtype=q.dtype)
    with _timed('mrattn_fwd', (3.0 * t + 3.0) * c * h * w * q.element_size() * n, detail=True):   # "work" = algorithmic bytes
        if q_scale is not None:
            _lib.call('mrefsr_mrattn_fwd_nhwc_scaled_f32', _p(q), _p(emb), _p(ass), _p(out), n, t, c, h * w, C.c_float(q_scale), _stream())
        else:
            _lib.call('mrefsr_mrattn_fwd_nhwc_bf16' if b16 else 'mrefsr_mrattn_fwd_nhwc_f32', _p(q), _p(emb), _p(ass), _p(out), n, t, c, h * w, _stream())
    return out


def mrattn_bwd(q, emb, ass, prob, g_out, t, t_major=False):
    _chk('mrattn_bwd', q, emb, ass, prob, g_out)
    n, c, h, w = q.shape
    c2 = ass.shape[1]
    g_q, g_emb, g_ass = torch.empty_like(q), torch.empty_like(emb), torch.empty_like(ass)
    _lib.call('mrefsr_mrattn_bwd_f32', _p(q), _p(emb), _p(ass), _p(prob), _p(g_out), _p(g_q), _p(g_emb), _p(g_ass), n, t,
              c, c2, h * w, 1 if t_major else 0, _stream())
    return g_q, g_emb, g_ass


def _chk_valid_bits(name, valid_bits, n):
    """valid_bits [N] int32 on the device: bit t of word n set = reference t of sample n is present"""
    _chk(name, valid_bits, dtype=torch.int32)
    if valid_bits is None or tuple(valid_bits.shape) != (n,):
        raise ValueError(f'{name}: valid_bits must be an int32 tensor of shape ({n},)')


def mrattn_fwd_masked(q, emb, ass, t, valid_bits, want_prob=True, t_major=False):
    """mrattn_fwd under per-sample reference masks: reference t of sample n takes part only if bit t of valid_bits[n] is set; its
    emb / ass are not read otherwise and its prob is exactly 0"""
    _chk('mrattn_fwd_masked', q, emb, ass)
    n, c, h, w = q.shape
    c2 = ass.shape[1]
    if emb.shape[0] != n * t or ass.shape[0] != n * t or emb.shape[1] != c:
        raise ValueError('mrattn_fwd_masked: inconsistent shapes')
    _chk_valid_bits('mrattn_fwd_masked', valid_bits, n)
    out = torch.empty((n, c2, h, w), device=q.device, dtype=torch.float32)
    prob = torch.empty((n, t, h, w), device=q.device, dtype=torch.float32) if want_prob else None
    _lib.call('mrefsr_mrattn_fwd_masked_f32', _p(q), _p(emb), _p(ass), _p(valid_bits), _p(out), _p(prob), n, t, c, c2, h * w,
              1 if t_major else 0, _stream())
    return out, prob


def mrattn_fwd_nhwc_masked(q, emb, ass, t, valid_bits, q_scale=None):
    """mrattn_fwd_nhwc under per-sample reference masks (valid_bits [N] int32, bit t = reference t of the sample is present)"""
    b16 = q.dtype == torch.bfloat16
    if q_scale is not None and b16:
        raise TypeError('mrattn_fwd_nhwc_masked: q_scale goes with fp32 tensors')
    _chk('mrattn_fwd_nhwc_masked', q, emb, ass, dtype=q.dtype if b16 else torch.float32)
    n, h, w, c = q.shape
    if tuple(emb.shape) != (n * t, h, w, c) or tuple(ass.shape) != (n * t, h, w, 2 * c):
        raise ValueError('mrattn_fwd_nhwc_masked: inconsistent shapes')
    _chk_valid_bits('mrattn_fwd_nhwc_masked', valid_bits, n)
    out = torch.empty((n, h, w, 2 * c), device=q.device, dtype=q.dtype)
    with _timed('mrattn_fwd', (3.0 * t + 3.0) * c * h * w * q.element_size() * n, detail=True):
        if b16:
            _lib.call('mrefsr_mrattn_fwd_nhwc_masked_bf16', _p(q), _p(emb), _p(ass), _p(valid_bits), _p(out), n, t, c, h * w, _stream())
        else:
            _lib.call('mrefsr_mrattn_fwd_nhwc_masked_f32', _p(q), _p(emb), _p(ass), _p(valid_bits), _p(out), n, t, c, h * w,
                      C.c_float(1.0 if q_scale is None else q_scale), _stream())
    return out


def mrattn_prob_nhwc(q, emb, t, valid_bits=None, q_scale=1.0):
    """the softmax weights of mrattn_fwd_nhwc / _masked alone: q [N,H,W,c], emb [t*N,H,W,c] (t-major) -> prob [N,H,W,t] fp32; an
    absent reference (valid_bits) gets exactly 0"""
    _chk('mrattn_prob_nhwc', q, emb)
    n, h, w, c = q.shape
    if tuple(emb.shape) != (n * t, h, w, c):
        raise ValueError('mrattn_prob_nhwc: inconsistent shapes')
    if valid_bits is not None:
        _chk_valid_bits('mrattn_prob_nhwc', valid_bits, n)
    prob = torch.empty((n, h, w, t), device=q.device, dtype=torch.float32)
    with _timed('mrattn_prob', ((t + 1.0) * c + t) * h * w * 4.0 * n, detail=True):   # "work" = algorithmic bytes, as mrattn_fwd
        _lib.call('mrefsr_mrattn_prob_nhwc_f32', _p(q), _p(emb), _p(valid_bits), _p(prob), n, t, c, h * w, C.c_float(q_scale), _stream())
    return prob


def mrattn_blend_conv(refs, prob, packed, bias, t, valid_bits=None, in_amax=None):
    """conv_ass applied to the softmax blend of the references (= the blend of conv_ass's results: the convolution is linear and the
    weights belong to the output pixel): refs [t*N,H,W,C] (t-major), prob [N,H,W,t], packed = the terms-16 PackedWeight of the
    [2C,C,3,3] weight, bias [2C] or None -> [N,H,W,2C].  in_amax: device word with max |refs| (None: no input scaling).
    Precondition: prob >= 0 and sum_t prob <= 1 at every pixel (softmax weights, mrattn_prob_nhwc): the fp16 range guard
    (conv_range_tripped) checks the staged references, and the blend stays below their maximum only under it"""
    _chk('mrattn_blend_conv', refs, prob, bias, in_amax)
    if packed.terms != 16:
        raise ValueError('mrattn_blend_conv: weights packed with terms=16 expected')
    tn, h, w, c = refs.shape
    n = prob.shape[0]
    if tn != n * t or tuple(prob.shape) != (n, h, w, t):
        raise ValueError('mrattn_blend_conv: inconsistent shapes')
    if packed.data.numel() != _lib.load().mrefsr_conv_packed_bytes(2 * c, c, 3, 16) or (bias is not None and bias.numel() != 2 * c):
        raise ValueError('mrattn_blend_conv: weight / bias do not belong to a C -> 2C 3x3 convolution')
    if valid_bits is not None:
        _chk_valid_bits('mrattn_blend_conv', valid_bits, n)
    out = torch.empty((n, h, w, 2 * c), device=refs.device, dtype=torch.float32)
    nby = (refs.numel() + prob.numel() + out.numel()) * 4.0 + 4.0 * c * 2 * c * 9
    with _timed('mrattn_blend_conv', 2.0 * n * h * w * c * 2 * c * 9, detail=True, nbytes=nby):
        _lib.call('mrefsr_mrattn_blend_conv_f32', _p(refs), _p(prob), _p(packed.data), _p(bias), _p(valid_bits), _p(in_amax),
                  _p(_range_flag(refs.device)), _p(out), n, t, h, w, c, C.c_float(packed.wscale), _stream())
    return out


def mrattn_bwd_masked(q, emb, ass, prob, g_out, t, valid_bits, t_major=False, out=None):
    """gradient of mrattn_fwd_masked -> (g_q, g_emb, g_ass); g_emb / g_ass of absent references are exact zeros.  out: the three
    buffers to write into (every element is written)"""
    _chk('mrattn_bwd_masked', q, emb, ass, prob, g_out)
    n, c, h, w = q.shape
    c2 = ass.shape[1]
    if (emb.shape[0] != n * t or ass.shape[0] != n * t or emb.shape[1] != c or tuple(prob.shape) != (n, t, h, w)
            or tuple(g_out.shape) != (n, c2, h, w)):
        raise ValueError('mrattn_bwd_masked: inconsistent shapes')
    _chk_valid_bits('mrattn_bwd_masked', valid_bits, n)
    g_q, g_emb, g_ass = _grad_triple('mrattn_bwd_masked', out, q, emb, ass)
    _lib.call('mrefsr_mrattn_bwd_masked_f32', _p(q), _p(emb), _p(ass), _p(prob), _p(g_out), _p(valid_bits), _p(g_q), _p(g_emb), _p(g_ass),
              n, t, c, c2, h * w, 1 if t_major else 0, _stream())
    return g_q, g_emb, g_ass


def _grad_triple(name, out, q, emb, ass):
    if out is None:
        return torch.empty_like(q), torch.empty_like(emb), torch.empty_like(ass)
    _chk(name, *out)
    if [tuple(o.shape) for o in out] != [tuple(v.shape) for v in (q, emb, ass)]:
        raise ValueError(f'{name}: out must be (g_q, g_emb, g_ass) shaped like (q, emb, ass)')
    return tuple(out)


# ------------------------------------------------------------------ fused_act / upfirdn2d
_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.float64: 3}


def fused_bias_act(x, bias, ref, act, grad, alpha, scale):
    """basicsr.ops.fused_act ext entry: empty bias / ref tensors mean 'absent'
    (fused_bias_act_kernel.cu:63-64)."""
    if x.dtype not in _DT:
        raise TypeError(f'fused_bias_act: unsupported dtype {x.dtype}')
    x = x.contiguous()
    bias = bias.contiguous() if bias is not None and bias.numel() else None
    ref = ref.contiguous() if ref is not None and ref.numel() else None
    _chk('fused_bias_act', x, bias, ref, dtype=x.dtype)
    step_b = 1
    for d in x.shape[2:]:
        step_b *= d
    out = torch.empty_like(x)
    _lib.call('mrefsr_fused_bias_act', _p(x), _p(bias), _p(ref), _p(out), C.c_int64(x.numel()), step_b,
              0 if bias is None else bias.numel(), int(act), int(grad), C.c_float(alpha), C.c_float(scale), _DT[x.dtype],
              _stream())
    return out


def tail_bilinear_add(y_nhwc, x, scale=4):
    """y_nhwc [B,H,W,C] (a channel slice of a wider tensor is fine) + F.interpolate(x [B,C,h,w], None, scale, 'bilinear', False) -> [B,C,H,W]
    (ref_mrapa_restoration_arch.py:132-137): one pass, torch's interpolation bits"""
    x = x.contiguous()
    _chk('tail_bilinear_add', x)
    if not y_nhwc.is_cuda or y_nhwc.dtype != torch.float32:
        raise TypeError(f'tail_bilinear_add: y on {y_nhwc.device}, {y_nhwc.dtype} (a CUDA fp32 tensor, rows may be padded)')
    b, c, h, w = x.shape
    if tuple(y_nhwc.shape) != (b, h * scale, w * scale, c) or y_nhwc.stride(3) != 1 or y_nhwc.stride(1) != y_nhwc.stride(2) * w * scale \
            or y_nhwc.stride(0) != y_nhwc.stride(1) * h * scale:
        raise ValueError(f'tail_bilinear_add: y {tuple(y_nhwc.shape)} / strides {y_nhwc.stride()} against x {tuple(x.shape)}')
    out = torch.empty((b, c, h * scale, w * scale), device=x.device, dtype=torch.float32)
    _lib.call('mrefsr_tail_bilinear_add_f32', _p(y_nhwc), _p(x), _p(out), b, c, h, w, scale, y_nhwc.stride(2), _stream())
    return out


def bias_act_res_(x, bias, slope, residual=None, pre=None):
    """in place on x [N,C,H,W] fp32: x = lrelu(x + bias[c] + pre, slope) (+ residual); `pre` [Np,C,H,W]
    is broadcast over N / Np groups.  slope 1 = identity, 0 = ReLU."""
    _chk('bias_act_res', x, bias, residual, pre)
    n, c = x.shape[0], x.shape[1]
    hw = x.numel() // (n * c)
    _lib.call('mrefsr_bias_act_res_f32', _p(x), _p(bias), _p(pre), C.c_int64(0 if pre is None else pre.shape[0]),
              _p(residual), _p(x), C.c_int64(n), c, C.c_int64(hw), C.c_float(slope), _stream())
    return x


_range_flags = {}  # device index -> int32[1]: set by conv_nhwc (terms=16) when an activation leaves the fp16 range


def _range_flag(device):
    f = _range_flags.get(device.index)
    if f is None:
        f = _range_flags[device.index] = torch.zeros(1, device=device, dtype=torch.int32)
    return f


_range_free = [False]


class range_free:
    """``with hip.range_free():`` -- the fp16 two-term kernels (|activation| < 65504) are replaced by their bf16 three-term
    twins (no range limit, ~1.5x slower) inside the block: convolutions pack / run with terms 6, the DCN takes its
    six-product split.  The re-run path after conv_range_tripped()."""

    def __enter__(self):
        self.saved = _range_free[0]
        _range_free[0] = True

    def __exit__(self, *exc):
        _range_free[0] = self.saved


def is_range_free():
    return _range_free[0]


def conv_range_tripped(reset=True):
    """True if any fp16-split kernel (terms=16 convolution, channels-last DCN) launched since the last call met a value
    outside the fp16 range (|x| > 65000, Inf or NaN).  One 4-byte readback (host sync) per device that ran such a kernel.
    MultiRefRestorationModel.test() / optimize_parameters() call it once per batch and re-run the batch on the range-free
    bf16 three-term split when it fires (archs/nhwc.range_free()).  The same word carries the "packed weights stale" bit of
    verify_packed(): read it with packed_stale()."""
    hit = False
    for f in _range_flags.values():
        v = int(f.item())
        if v & _STALE_BIT:
            _packed.stale = True
        if v & 1:
            hit = True
        if v and reset:
            f.zero_()
    return hit


def check_conv_range(reset=True):
    """Raise if conv_range_tripped(): for callers that drive the kernels directly and want the event as an error."""
    if conv_range_tripped(reset):
            raise FloatingPointError('mrefsr_conv_nhwc_f32 (terms=16) / mrefsr_dcn_fwd_f32: an activation exceeded the fp16 range '
                                     '(|x| > 65000 or NaN); rerun with MREFSR_CONV_TERMS=6 MREFSR_DCN_TERMS=6 (bf16 three-term '
                                     'splits, no range limit)')


class PackedWeight:
    """packed split fragments + the power-of-two scale they carry (terms == 16; 1.0 otherwise)"""
    __slots__ = ('data', 'wscale', 'terms')

    def __init__(self, data, wscale, terms):
        self.data, self.wscale, self.terms = data, wscale, terms


_STALE_BIT = 2


class _Fingerprint:
    """a parameter as verify() checks it: stamp and size, the checksum taken when it was packed (a device word), and the one-row
    table and counter of that launch (they live as long as the launch may)"""
    __slots__ = ('ref', 'stamp', 'numel', 'sum', 'row', 'done')


class _Fold:
    """a derived entry of _PackedWeights: the sources (weak; None where a bias is absent) with their stamps, the packed composed weight
    and the composed bias"""
    __slots__ = ('refs', 'stamps', 'packed', 'bias')


class _PackedWeights:
    """Packed copies of the inference path's convolution weights by (id(parameter), slice, terms), each good for one param_stamp():
    re-packed when the parameter is modified through autograd-visible ops, re-allocated or replaced.  Unlike the training tables,
    which key by storage because autograd hands back new Python handles, this cache keys by the parameter object -- and it alone
    also catches writes through ``p.data``, which move no stamp, on the device: every parameter is fingerprinted when packed (a
    one-row checksum launch on the stream that has just packed it: such a write between this packing and the next verify() is
    then a mismatch, not part of the reference) and again by verify(); the verdict travels in the range flag's word (no extra
    readback), conv_range_tripped() leaves it in ``stale``, and the model then drops the cache and repeats the pass."""

    def __init__(self):
        self.copies, self.prints = {}, {}        # (id(weight), slice, terms) -> _Packed; id(weight) -> _Fingerprint
        self.folds = {}                          # (ids of w3x3, b3x3, w1x1, b1x1, cin_offset, terms) -> _Fold (get_fold)
        self.order, self.dirty = [], True        # the device table over self.prints, rebuilt lazily: its rows, out of date
        self.table = self.sums = self.done = self.ref = None
        self.stale, self.epoch = False, 0

    def get(self, weight, cin_slice=None, terms=6):
        """cached conv_pack_weight(weight[:, a:b])"""
        key = (id(weight), cin_slice, terms)
        hit = self.copies.get(key)
        if hit is not None and param_stamp(hit.ref()) == hit.stamp:
            return hit.packed
        if len(self.copies) > 4096:   # entries of parameters that no longer exist
            for k in [k for k, v in self.copies.items() if v.ref() is None]:
                del self.copies[k]
        w = weight.detach()
        if cin_slice is not None:
            w = w[:, cin_slice[0]:cin_slice[1]]
        hit = self.copies[key] = _Packed(weight, conv_pack_weight(w.contiguous(), terms), param_stamp(weight))
        self._fingerprint(weight, hit.ref, hit.stamp)
        return hit.packed

    def _fingerprint(self, weight, ref, stamp):
        """take ``weight``'s checksum on the stream that has just read it, as what verify() compares with from now on"""
        fp = self.prints[id(weight)] = _Fingerprint()
        fp.ref, fp.stamp, fp.numel, dev = ref, stamp, weight.numel(), weight.device
        fp.row = torch.tensor([fp.stamp.ptr, fp.numel], dtype=torch.int64).to(dev)
        fp.sum = torch.zeros(1, dtype=torch.int64, device=dev)
        fp.done = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.call('mrefsr_weights_checksum', _p(fp.row), 1, _p(fp.sum), _p(fp.done), None, None, 0, _stream())
        self.dirty = True

    def get_fold(self, w3x3, b3x3, w1x1, b1x1, cin_offset, terms):
        """(packed W', b') of a 1x1 convolution (columns cin_offset.. of ``w1x1``) applied behind a 3x3 one: conv_compose_1x1_3x3 of
        the four parameters (either bias may be None), W' packed with ``terms`` -- a DERIVED entry, keyed by its sources and good
        while every source's param_stamp() stands.  All sources, the biases too, are fingerprinted for verify(): none of them
        need have a packed copy of its own.  A source that already carries a fingerprint of its current stamp keeps it (the older
        reference is the stricter one: a ``.data`` write since then still reads as a mismatch)."""
        srcs = (w3x3, b3x3, w1x1, b1x1)
        key = tuple(0 if s is None else id(s) for s in srcs) + (cin_offset, terms)
        hit = self.folds.get(key)
        if hit is not None and all(r is None or param_stamp(r()) == st for r, st in zip(hit.refs, hit.stamps)):
            return hit.packed, hit.bias
        if len(self.folds) > 256:   # entries of parameters that no longer exist
            for k in [k for k, v in self.folds.items() if any(r is not None and r() is None for r in v.refs)]:
                del self.folds[k]
        w, b = conv_compose_1x1_3x3(w1x1.detach(), w3x3.detach(), None if b3x3 is None else b3x3.detach(),
                                    None if b1x1 is None else b1x1.detach(), cin_offset)
        hit = self.folds[key] = _Fold()
        hit.refs = tuple(None if s is None else weakref.ref(s) for s in srcs)
        hit.stamps = tuple(None if s is None else param_stamp(s) for s in srcs)
        hit.packed, hit.bias = conv_pack_weight(w, terms), b
        for s, r, st in zip(srcs, hit.refs, hit.stamps):
            have = None if s is None else self.prints.get(id(s))
            if s is not None and not (have is not None and have.ref() is s and have.stamp == st):
                self._fingerprint(s, r, st)
        return hit.packed, hit.bias

    def verify(self, device=None):
        """One launch: fingerprint every parameter with a cached packed copy and raise the stale bit where it differs from the
        fingerprint taken at packing time.  No synchronisation; the bit is read with the range flag (conv_range_tripped(), then
        packed_stale()).  Call it once per forward pass, before the convolutions."""
        # (a parameter whose stamp moved is re-packed, and re-fingerprinted, by the pass that follows: it leaves the check)
        moved = [wid for wid, fp in self.prints.items() if fp.ref() is not None and param_stamp(fp.ref()) != fp.stamp]
        for wid in moved:
            del self.prints[wid]
        if not self.prints:
            self.dirty |= bool(moved)
            return
        device = device or torch.device('cuda', torch.cuda.current_device())
        live = {wid: fp for wid, fp in self.prints.items() if fp.ref() is not None}
        if moved or self.dirty or self.table is None or len(live) != len(self.order):
            self.prints, self.order, n = live, list(live.values()), len(live)
            self.table = torch.tensor([v for fp in self.order for v in (fp.stamp.ptr, fp.numel)], dtype=torch.int64).view(-1, 2).to(device)
            self.sums = torch.zeros(n, dtype=torch.int64, device=device)
            self.done = torch.zeros(n, dtype=torch.int32, device=device)
            self.ref = torch.cat([fp.sum for fp in self.order]) if n else None   # the fingerprints taken at packing time
            self.dirty = False
        if self.order:
            _lib.call('mrefsr_weights_checksum', _p(self.table), len(self.order), _p(self.sums), _p(self.done), _p(self.ref),
                      _p(_range_flag(device)), _STALE_BIT, _stream())

    def take_stale(self, reset=True):
        """True if verify() found a parameter that no longer matches its packed copy (seen at the last conv_range_tripped()
        readback); the caller drops the cache (invalidate_packed()) and repeats the pass."""
        seen, self.stale = self.stale, self.stale and not reset
        return seen

    def clear(self):
        """drop every cached packed weight (and let hipGraph captures notice): call after editing parameters through ``.data``"""
        self.copies.clear()
        self.folds.clear()
        self.prints, self.order, self.dirty, self.table, self.ref = {}, [], True, None, None
        self.epoch += 1


_packed = _PackedWeights()
packed_weight, verify_packed, packed_stale, invalidate_packed = _packed.get, _packed.verify, _packed.take_stale, _packed.clear
packed_fold = _packed.get_fold


def packed_epoch():
    return _packed.epoch


def conv_pack_weight(weight, terms=6):
    """weight [Cout,Cin,k,k] fp32 (k = 1 or 3) -> PackedWeight (split fragments as a uint8 tensor) for conv_nhwc.
    terms=16 (fp16 two-term split) scales the weights by 2^s with max|w| * 2^s in [2^13, 2^14): one host
    sync per packing (the result is cached per parameter version by packed_weight)."""
    import math
    _chk('conv_pack_weight', weight)
    co, ci, kh, kw = weight.shape
    if kh != kw or kh not in (1, 3):
        raise ValueError('conv_pack_weight: 1x1 or 3x3 kernels only')
    wscale = 1.0
    if terms == 17 and kh != 3:
        raise ValueError('conv_pack_weight: terms=17 (Winograd F(2x2, 3x3)) is for 3x3 kernels')
    if terms in (16, 17):   # 17: the Winograd form of 16 -- |G g G^T| <= 2.25 max|w| stays inside fp16 under the same scale
        amax = float(weight.abs().max().item())
        if not math.isfinite(amax):
            raise ValueError('conv_pack_weight: non-finite weights')
        wscale = 2.0 ** (13 - math.floor(math.log2(amax))) if amax > 0 else 1.0
    nbytes = _lib.load().mrefsr_conv_packed_bytes(co, ci, kh, terms)
    packed = torch.empty(nbytes, device=weight.device, dtype=torch.uint8)
    _lib.call('mrefsr_conv_pack_weight_f32', _p(weight), _p(packed), co, ci, kh, terms, C.c_float(wscale), _stream())
    return PackedWeight(packed, wscale, terms)


def conv_compose_1x1_3x3(w1x1, w3x3, b3x3=None, b1x1=None, cin_offset=0):
    """The 3x3 convolution that equals ``w3x3`` [Cmid,Cin,3,3] (+ b3x3) followed by the 1x1 convolution with columns
    cin_offset .. cin_offset + Cmid of ``w1x1`` [Cout,ld(,1,1)] (+ b1x1): -> (W' [Cout,Cin,3,3], b' [Cout] or None when both biases
    are None).  fp64 sums in a fixed order, rounded once (csrc/conv_fold.hip); W' packs like any weight (conv_pack_weight)."""
    _chk('conv_compose_1x1_3x3', w1x1, w3x3, b3x3, b1x1)
    co, ld = w1x1.shape[0], w1x1.shape[1]
    cm, ci = w3x3.shape[0], w3x3.shape[1]
    if w1x1.numel() != co * ld or tuple(w3x3.shape[2:]) != (3, 3) or cin_offset < 0 or cin_offset + cm > ld:
        raise ValueError(f'conv_compose_1x1_3x3: w1x1 {tuple(w1x1.shape)} (columns from {cin_offset}) behind w3x3 {tuple(w3x3.shape)}')
    if (b3x3 is not None and b3x3.numel() != cm) or (b1x1 is not None and b1x1.numel() != co):
        raise ValueError('conv_compose_1x1_3x3: bias sizes')
    out_w = torch.empty((co, ci, 3, 3), device=w3x3.device, dtype=torch.float32)
    out_b = None if (b3x3 is None and b1x1 is None) else torch.empty(co, device=w3x3.device, dtype=torch.float32)
    _lib.call('mrefsr_conv_compose_1x1_3x3_f32', _p(w1x1), C.c_int64(ld), cin_offset, _p(w3x3), _p(b3x3), _p(b1x1), _p(out_w), _p(out_b),
              co, cm, ci, _stream())
    return out_w, out_b


def conv_pack_view(weight, cin_slice=None, terms=6, dgrad=False, wscale=1.0):
    """Packed fragments of weight[:, a:b] (``cin_slice`` = (a, b), default all input channels) read in place -- no slicing
    copy -- or, with ``dgrad``, of the operator of the convolution's input gradient w.r.t. those channels (output channels
    b - a, input channels Cout, taps point-mirrored): ``conv_nhwc(g_out, that, None, b - a, k)`` is d loss / d x[..., a:b].
    No host synchronisation: terms 16 (fp16 two-term split) takes the power-of-two ``wscale`` from the caller (max|w| * wscale
    must stay below 65504; conv_pack_weight derives it from the weight's amax with a readback)."""
    _chk('conv_pack_view', weight)
    co, ci, kh, kw = weight.shape
    if kh != kw or kh not in (1, 3):
        raise ValueError('conv_pack_view: 1x1 or 3x3 kernels only')
    if terms not in (6, 1, 16):
        raise ValueError('conv_pack_view: terms 6, 1 or 16')
    pw, j = conv_pack_plan(weight, cin_slice, terms, dgrad, wscale)
    conv_pack_one(j)
    return pw


def conv_pack_one(j):
    """run one mrefsr_conv_pack_job by itself"""
    _lib.call('mrefsr_conv_pack_weight_view_f32', C.c_void_p(j.weight), C.c_void_p(j.packed), j.Cout, j.Cin, j.ksize, j.terms, C.c_float(j.wscale),
              C.c_int64(j.stride_o), C.c_int64(j.stride_i), j.flip, _stream())


def conv_pack_plan(weight, cin_slice=None, terms=6, dgrad=False, wscale=1.0):
    """(PackedWeight with an unfilled buffer, the mrefsr_conv_pack_job that fills it): conv_pack_view's arguments as a table entry
    for conv_pack_multi.  The job holds raw addresses: the caller keeps ``weight`` and the PackedWeight alive."""
    co, ci, kh, kw = weight.shape
    if not weight.is_contiguous():
        raise ValueError('conv_pack_plan: contiguous OIHW weight expected')
    if terms != 16:
        wscale = 1.0
    a, b = cin_slice if cin_slice is not None else (0, ci)
    taps = kh * kw
    po, pi, so, si = (b - a, co, taps, ci * taps) if dgrad else (co, b - a, ci * taps, taps)
    nbytes = _lib.load().mrefsr_conv_packed_bytes(po, pi, kh, terms)
    packed = torch.empty(nbytes, device=weight.device, dtype=torch.uint8)
    # dgrad = 'T': the transposed operator WITHOUT the point mirror (d columns = W^T . g_out of a deformable convolution: the taps
    # keep their places, mrefsr_dcn_bwd_data_f32)
    job = _lib.ConvPackJob(weight.data_ptr() + 4 * a * taps, packed.data_ptr(), so, si, po, pi, kh, terms, 1 if dgrad is True else 0, wscale)
    return PackedWeight(packed, wscale, terms), job


def conv_pack_table(jobs, device):
    """device copy of a list of mrefsr_conv_pack_job (a synchronous upload: build it when the set of weights changes, not per step)"""
    arr = (_lib.ConvPackJob * len(jobs))(*jobs)
    return torch.frombuffer(bytearray(arr), dtype=torch.uint8).to(device)


def conv_pack_multi(table, n_jobs):
    """run the n_jobs packings of a conv_pack_table in one launch; a weight that no longer fits the fp16 range under the scale
    of its job raises the range flag (conv_range_tripped())"""
    _lib.call('mrefsr_conv_pack_weights_multi_f32', _p(table), n_jobs, _p(_range_flag(table.device)), _stream())


# ------------------------------------------------------------------ the parameter update (csrc/optim.hip): Adam and the EMA of net_g
_OPTIM_CHUNK = 1024   # elements per chunk of csrc/optim.hip (mrefsr_optim_job_chunks(n) = ceil((n + 3) / 1024), 0 for n = 0)


class OptimTable:
    """a table of mrefsr_optim_job in device memory and the addresses it was built from (``key``); it holds no tensor alive: a
    table is only ever used with the tensors whose addresses have just been compared with its key"""
    __slots__ = ('key', 'table', 'n_jobs')


def optim_table(ps, gs=None, ms=None, vs=None, emas=None, groups=None, cached=None, need_moments=True):
    """The job table of ema_multi / adam_multi over the parameters ``ps``: per parameter its gradient, moments and EMA copy (each
    list may be None, each entry may be None) and its index into the Adam groups.  ``cached``: the table of the call before; it
    is returned as it is when no address, size or group has moved, otherwise a new one is built and uploaded (a synchronous
    copy of 56 bytes per tensor: not under hipGraph capture).  ``need_moments`` False: a table of gradients alone, for
    grad_norm_multi / grad_scale_multi in front of an optimiser that is not adam_multi (which takes no step without moments)."""
    n = len(ps)
    none = [None] * n
    gs, ms, vs, emas = gs or none, ms or none, vs or none, emas or none
    groups = groups or [0] * n
    key = tuple((p.data_ptr(), 0 if g is None else g.data_ptr(), 0 if m is None else m.data_ptr(), 0 if v is None else v.data_ptr(),
                 0 if e is None else e.data_ptr(), p.numel(), gi) for p, g, m, v, e, gi in zip(ps, gs, ms, vs, emas, groups))
    if cached is not None and cached.key == key:
        return cached
    if n == 0:
        raise ValueError('optim_table: no tensors')
    import numpy as np
    device = ps[0].device
    old = cached.key if cached is not None and len(cached.key) == n else none
    for row, was, p, g, m, v, e in zip(key, old, ps, gs, ms, vs, emas):
        if row == was:   # (checked when the table before this one was built)
            continue
        for k, t in enumerate((p, g, m, v, e)):
            if t is not None and (was is None or row[k] != was[k] or row[5] != was[5]):
                _chk('optim_table', t)
                if t.numel() != row[5] or t.device != device:
                    raise ValueError('optim_table: a gradient, moment or EMA tensor does not match its parameter (size / device)')
        if need_moments and g is not None and (m is None or v is None):
            raise ValueError('optim_table: a gradient without both moments')
    rows = np.array(key, dtype=np.int64)                    # mrefsr_optim_job: five addresses, n, then first_chunk | group << 32
    chunks = np.where(rows[:, 5] > 0, (rows[:, 5] + 3 + _OPTIM_CHUNK - 1) // _OPTIM_CHUNK, 0)   # mrefsr_optim_job_chunks
    first = np.cumsum(chunks) - chunks
    if int(first[-1] + chunks[-1]) >= 2 ** 31:
        raise ValueError('optim_table: too many elements')
    rows[:, 6] = first | ((rows[:, 6] & 0xFFFFFFFF) << 32)
    tab = OptimTable()
    tab.key, tab.n_jobs = key, n
    tab.table = torch.from_numpy(rows).to(device)
    return tab


def _written(tensors):
    # the kernels write through raw pointers: autograd's version counters are moved by hand, so that everything keyed by them
    # (the packed weight copies of packed_weight / nhwc_train, verify_packed, the inference graph's key) sees the change
    torch.autograd.graph.increment_version(tensors)


def ema_multi(tab, decay, emas):
    """ema = decay * ema + (1 - decay) * p for every job of ``tab`` that has an EMA tensor (``emas``: those tensors), one launch;
    decay 0 copies p bit for bit"""
    decay = float(decay)
    if not 0.0 <= decay <= 1.0:
        raise ValueError(f'ema_multi: decay {decay} outside [0, 1]')
    _lib.call('mrefsr_ema_multi_f32', _p(tab.table), tab.n_jobs, C.c_float(decay), C.c_float(1.0 - decay), _stream())
    _written(emas)


class GradClipState:
    """mrefsr_grad_clip_state in device memory (``buf``: 24 bytes as six fp32 words) with 0-dim views of its fields -- the
    unclipped ``total_norm``, ``coef``, ``found_inf`` (fp32 0 / 1: torch's fused Adam takes it as optimizer.found_inf) and
    ``skipped`` (int64) -- and the workspace of the norm's per-block partial sums.  Nothing is read back here."""
    __slots__ = ('buf', 'total_norm', 'coef', 'found_inf', 'skipped', 'workspace')

    def __init__(self, device):
        self.buf = torch.zeros(C.sizeof(_lib.GradClipState) // 4, device=device, dtype=torch.float32)
        self.total_norm, self.coef, self.found_inf = self.buf[0], self.buf[1], self.buf[2]
        self.skipped = self.buf[4:6].view(torch.int64)[0]
        self.workspace = torch.empty(_lib.load().mrefsr_grad_norm_workspace_bytes() // 8, device=device, dtype=torch.float64)


def grad_norm_multi(tab, state, max_norm=0.0, skip=False):
    """The global L2 norm of every gradient of ``tab`` into ``state`` (a GradClipState), two launches: the per-block sums of
    squares and the one-block finalize that also writes coef = min(max_norm / (total_norm + 1e-6), 1) (``max_norm`` <= 0: no
    clipping, 1), found_inf, and counts a skipped step when ``skip`` and the norm is not finite.  Fixed summation order."""
    max_norm = float(max_norm)
    if not math.isfinite(max_norm):
        raise ValueError(f'grad_norm_multi: max_norm {max_norm} is not finite')
    ws = state.workspace
    _lib.call('mrefsr_grad_sqnorm_multi_f32', _p(tab.table), tab.n_jobs, _p(ws), ws.numel() * 8, _stream())
    _lib.call('mrefsr_grad_norm_finalize_f32', _p(ws), ws.numel() * 8, C.c_float(max_norm), int(bool(skip)), _p(state.buf), _stream())


def grad_scale_multi(tab, state, grads):
    """g = fl32(g * state.coef) in place for every gradient of ``tab`` (``grads``: those tensors), one launch: the second half
    of torch's clip_grad_norm_, for an optimiser that reads the gradient tensors (adam_multi's ``clip=`` needs no such pass)"""
    _lib.call('mrefsr_grad_scale_multi_f32', _p(tab.table), tab.n_jobs, _p(state.buf), _stream())
    _written(grads)


def adam_multi(tab, groups, written, ema_decay=0.0, clip=None, skip=False):
    """torch.optim.Adam's step for every job of ``tab`` that has a gradient, one launch: ``groups`` = [(lr, beta1, beta2, eps,
    weight_decay, step), ...] with ``step`` counting this update; jobs with an EMA tensor get its update with ``ema_decay`` in
    the same pass.  ``written``: the parameters and EMA tensors the launch writes (the moments carry no version anyone reads).
    ``clip``: the GradClipState that grad_norm_multi has just filled for this table -- the gradients enter as fl32(g * coef)
    without being written, the step counts are taken less ``clip.skipped``, and with ``skip`` a non-finite norm leaves
    parameters and moments as they are (the EMA update is still made)."""
    ema_decay = float(ema_decay)
    if not 0.0 <= ema_decay <= 1.0:
        raise ValueError(f'adam_multi: ema_decay {ema_decay} outside [0, 1]')
    if not groups or any(int(g[5]) < 1 for g in groups):
        raise ValueError('adam_multi: no groups / a step count below 1')
    arr = (_lib.AdamGroup * len(groups))(*[_lib.AdamGroup(*(float(x) for x in g[:5]), int(g[5])) for g in groups])
    dev = torch.frombuffer(bytearray(arr), dtype=torch.uint8).to(tab.table.device)
    if clip is None:
        if skip:
            raise ValueError('adam_multi: skip needs the clip state of grad_norm_multi')
        _lib.call('mrefsr_adam_multi_f32', _p(tab.table), tab.n_jobs, _p(dev), len(groups), C.c_float(ema_decay), C.c_float(1.0 - ema_decay),
                  _stream())
    else:
        _lib.call('mrefsr_adam_multi_clip_f32', _p(tab.table), tab.n_jobs, _p(dev), len(groups), C.c_float(ema_decay),
                  C.c_float(1.0 - ema_decay), _p(clip.buf), int(bool(skip)), _stream())
    _written(written)


# ------------------------------------------------------------------ R1 regularisation of the discriminator (csrc/gan_reg.hip)
def r1_lane_squares(n):
    """L of r1_sqnorm's error bound ((L + 1) / 2 + 2) 2^-24: the squares one lane adds for rows of ``n`` elements"""
    blocks = _lib.load().mrefsr_r1_sqnorm_row_blocks(n)
    if blocks <= 0:
        raise ValueError(f'r1_lane_squares: n = {n}')
    chunks = (n + 3 + _OPTIM_CHUNK - 1) // _OPTIM_CHUNK
    return 4 * ((chunks + blocks - 1) // blocks)


def _r1_rows(name, g):
    if g.dim() < 1 or g.numel() == 0:
        raise ValueError(f'{name}: a non-empty [B, ...] tensor expected, got {tuple(g.shape)}')
    return g.shape[0], g.numel() // g.shape[0]


def r1_sqnorm(g):
    """g [B, ...] (contiguous fp32, any 4-byte alignment) -> [B] fp32: g.pow(2).view(B, -1).sum(1) of r1_penalty
    (basicsr/losses/losses.py:404), added in a fixed order -- fp32 per lane, double across lanes, waves and blocks; two launches,
    no atomics, the same bits from run to run"""
    _chk('r1_sqnorm', g)
    b, n = _r1_rows('r1_sqnorm', g)
    nbytes = _lib.load().mrefsr_r1_sqnorm_workspace_bytes(b, n)
    if nbytes <= 0:
        raise ValueError(f'r1_sqnorm: unsupported shape {tuple(g.shape)}')
    ws = torch.empty(nbytes // 8, device=g.device, dtype=torch.float64)
    out = torch.empty(b, device=g.device, dtype=torch.float32)
    _lib.call('mrefsr_r1_sqnorm_f32', _p(g), b, n, _p(out), _p(ws), nbytes, _stream())
    return out


def r1_sqnorm_bwd(g, gs, out=None):
    """the backward of r1_sqnorm towards g: fl32(fl32(2 gs[b]) g[b][i]) in g's shape, the bits of torch's g * (2 * gs).view(B, 1);
    one launch.  ``out``: a contiguous fp32 tensor of g's shape to write into (any 4-byte alignment)"""
    _chk('r1_sqnorm_bwd', g, gs, out)
    b, n = _r1_rows('r1_sqnorm_bwd', g)
    if gs.shape != (b, ):
        raise ValueError(f'r1_sqnorm_bwd: gs {tuple(gs.shape)} for g {tuple(g.shape)}')
    if out is not None and out.shape != g.shape:
        raise ValueError(f'r1_sqnorm_bwd: out {tuple(out.shape)} for g {tuple(g.shape)}')
    gg = torch.empty_like(g) if out is None else out
    _lib.call('mrefsr_r1_sqnorm_bwd_f32', _p(g), _p(gs), b, n, _p(gg), _stream())
    return gg


# ------------------------------------------------------------------ x8 geometric self-ensemble of test() (csrc/selfens.hip)
def dihedral_expand(src, tr, outer=1):
    """src [outer * inner, C, H, W] (contiguous fp32; the leading axis outer-major, e.g. the k-major reference stack with outer = K)
    -> [outer * 4 * inner, C, Ho, Wo], (Ho, Wo) = (W, H) if tr else (H, W): row (o * 4 + j) * inner + i is copy j of row o * inner + i,
    copy j = flip(-1) if j & 1, then flip(-2) if j & 2, then transpose(-1, -2) if tr.  A pure copy (the bits of the torch
    statement); one launch"""
    _chk('dihedral_expand', src)
    if tr not in (0, 1):
        raise ValueError(f'dihedral_expand: tr {tr!r} is not 0 or 1')
    if src.dim() != 4 or src.numel() == 0 or not isinstance(outer, int) or outer < 1 or src.shape[0] % outer:
        raise ValueError(f'dihedral_expand: a non-empty [outer * inner, C, H, W] tensor expected, got {tuple(src.shape)} with outer = {outer!r}')
    n, c, h, w = src.shape
    dst = torch.empty((4 * n, c, w, h) if tr else (4 * n, c, h, w), device=src.device, dtype=torch.float32)
    with _timed('dihedral_expand', detail=True, nbytes=4.0 * (src.numel() + dst.numel())):
        _lib.call('mrefsr_dihedral_expand_f32', _p(src), _p(dst), outer, n // outer, c, h, w, int(tr), _stream())
    return dst


def dihedral_merge(a, b):
    """a [4 * N, C, H, W], b [4 * N, C, W, H] (contiguous fp32; row j * N + n is the output of copy j of sample n in the
    untransposed / the transposed group) -> [N, C, H, W]: the eight outputs with their transforms undone, added in fp32 as
    (((((((a0 + a1) + a2) + a3) + b0) + b1) + b2) + b3) * 0.125 (the bits of that chain in torch); one launch"""
    _chk('dihedral_merge', a, b)
    if a.dim() != 4 or a.numel() == 0 or a.shape[0] % 4 or tuple(b.shape) != (a.shape[0], a.shape[1], a.shape[3], a.shape[2]):
        raise ValueError(f'dihedral_merge: a [4 N, C, H, W] and b [4 N, C, W, H] expected, got {tuple(a.shape)} and {tuple(b.shape)}')
    n4, c, h, w = a.shape
    out = torch.empty((n4 // 4, c, h, w), device=a.device, dtype=torch.float32)
    with _timed('dihedral_merge', detail=True, nbytes=4.0 * (a.numel() + b.numel() + out.numel())):
        _lib.call('mrefsr_dihedral_merge_f32', _p(a), _p(b), _p(out), n4 // 4, c, h, w, _stream())
    return out


# ------------------------------------------------------------------ colour correction of test() outputs (csrc/color_fix.hip)
COLOR_FIX_MAX_LEVELS = 5


def _color_fix_args(name, x, s, sizes, min_pixels=1):
    """the checks of both colour-fix calls, all on the host before anything is launched -> (B, C, H, W, the [B,2] int32 device table
    or None).  sizes: None or B pairs (h_b, w_b) of ints with 1 <= h_b <= H, 1 <= w_b <= W"""
    _chk(name, x, s)
    if x.dim() != 4 or x.numel() == 0 or s.shape != x.shape:
        raise ValueError(f'{name}: two non-empty [B,C,H,W] tensors of one shape expected, got {tuple(x.shape)} and {tuple(s.shape)}')
    b, c, h, w = x.shape
    rects = [(h, w)] * b
    table = None
    if sizes is not None:
        rects = [tuple(int(v) for v in tuple(r)[:2]) for r in sizes]
        if len(rects) != b or any(len(r) != 2 for r in rects):
            raise ValueError(f'{name}: sizes: {b} pairs (h_b, w_b) expected for a batch of {b}, got {sizes!r}')
        for hb, wb in rects:
            if not (1 <= hb <= h and 1 <= wb <= w):
                raise ValueError(f'{name}: sizes: ({hb}, {wb}) is not inside the {h} x {w} planes (1 <= h_b <= H, 1 <= w_b <= W)')
    for hb, wb in rects:
        if hb * wb < min_pixels:
            raise ValueError(f'{name}: a valid rectangle of {hb} x {wb} = {hb * wb} pixel(s) has no unbiased variance '
                             f'(at least {min_pixels} pixels needed)')
    if sizes is not None:
        table = torch.tensor(rects, dtype=torch.int32).to(x.device)
    return b, c, h, w, table


def color_fix_wavelet(x, s, sizes=None, levels=5):
    """x (the output), s (the colour source) [B,C,H,W] contiguous fp32 -> x + low_L(s - x) = high_L(x) + low_L(s), L = levels in
    1..5: low_i = low_{i-1} filtered with [1,2,1]^T [1,2,1] / 16 at dilation 2^(i-1), replicate padding at every stage
    (color_fix.wavelet_color_fix_torch states it).  sizes: None or B pairs (h_b, w_b): the top-left rectangle that is the image of
    sample b; outside it the result is x's bits.  One launch; the inputs are only read; the same bits from call to call"""
    if isinstance(levels, bool) or not isinstance(levels, int) or not 1 <= levels <= COLOR_FIX_MAX_LEVELS:
        raise ValueError(f'color_fix_wavelet: levels {levels!r} is not an int in 1..{COLOR_FIX_MAX_LEVELS}')
    b, c, h, w, table = _color_fix_args('color_fix_wavelet', x, s, sizes)
    out = torch.empty_like(x)
    with _timed('color_fix_wavelet', detail=True, nbytes=12.0 * x.numel()):
        _lib.call('mrefsr_color_fix_wavelet_f32', _p(x), _p(s), _p(out), b, c, h, w, _p(table), levels, _stream())
    return out


def color_fix_adain(x, s, sizes=None):
    """x, s [B,C,H,W] contiguous fp32 -> (x - mu_x) (sigma_s / sigma_x) + mu_s per (b, c) plane, mu the mean and sigma = sqrt(var +
    1e-5) with the unbiased variance over the plane's valid rectangle (color_fix.adain_color_fix_torch states it); sizes as in
    color_fix_wavelet; a rectangle of one pixel is a ValueError.  Two launches, statistics and the expression in double, one
    rounding to fp32; fixed summation order, no atomics, nothing read back"""
    b, c, h, w, table = _color_fix_args('color_fix_adain', x, s, sizes, min_pixels=2)
    need = _lib.load().mrefsr_color_fix_adain_workspace_bytes(b, c, h, w)
    if need <= 0:
        raise ValueError(f'color_fix_adain: unsupported shape {tuple(x.shape)} (B C <= 65535, H W <= 2^30)')
    ws, ticket = _det_scratch(x.device, need)
    out = torch.empty_like(x)
    with _timed('color_fix_adain', detail=True, nbytes=16.0 * x.numel()):
        _lib.call('mrefsr_color_fix_adain_f32', _p(x), _p(s), _p(out), b, c, h, w, _p(table), _p(ws), C.c_int64(need), _p(ticket), _stream())
    return out


# ------------------------------------------------------------------ homography views and the matcher probe (csrc/warp.hip)
WARP_INTERP = {'bilinear': 0, 'bicubic': 1}
MATCH_STATS_MAX_THRESHOLDS = 4


def _homographies(name, m, n, device):
    """m: one 3 x 3 matrix or n of them ([3,3], [n,3,3] or [n,9]; a tensor or anything torch.as_tensor takes) -> [n,9] float64 on
    ``device`` (a host value is one small upload)"""
    m = torch.as_tensor(m)
    if not (m.is_floating_point() or m.dtype in (torch.int32, torch.int64)):
        raise TypeError(f'{name}: a real matrix expected, got {m.dtype}')
    if m.dim() == 2 and tuple(m.shape) == (3, 3):
        m = m.expand(n, 3, 3)
    if tuple(m.shape) not in ((n, 3, 3), (n, 9)):
        raise ValueError(f'{name}: one 3 x 3 matrix or {n} of them ([{n},3,3] / [{n},9]) expected for a batch of {n}, got {tuple(m.shape)}')
    return m.reshape(n, 9).to(device=device, dtype=torch.float64).contiguous()


def warp_perspective(x, S, out_size=None, interp='bicubic', clamp=False):
    """x [N,C,H,W] contiguous fp32 -> [N,C,Ho,Wo] (out_size = (Ho, Wo), default (H, W)): the projective view of every image under
    its SAMPLING matrix S[n] (destination -> source, integer pixel coordinates: out(xo, yo) = x at S (xo, yo, 1), the M^-1 of
    cv2.warpPerspective; views.py makes such matrices).  S: one 3 x 3 matrix or N of them, float64; a host value is uploaded (one
    small copy).  interp 'bicubic' (cubic convolution, A = -0.75) or 'bilinear'; taps outside the image are 0; clamp: the result
    clamped to [0, 1].  One launch; no backward (an input-side operator).  csrc/warp.hip states the arithmetic"""
    _chk('warp_perspective', x)
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError(f'warp_perspective: a non-empty [N,C,H,W] tensor expected, got {tuple(x.shape)}')
    if interp not in WARP_INTERP:
        raise ValueError(f'warp_perspective: interp {interp!r} is not one of {", ".join(WARP_INTERP)}')
    if not isinstance(clamp, bool):
        raise ValueError(f'warp_perspective: clamp {clamp!r} is not true or false')
    n, c, h, w = x.shape
    ho, wo = (h, w) if out_size is None else (int(v) for v in out_size)
    if ho < 1 or wo < 1:
        raise ValueError(f'warp_perspective: out_size {out_size!r} is not a pair of positive sizes')
    s = _homographies('warp_perspective', S, n, x.device)
    out = torch.empty((n, c, ho, wo), device=x.device, dtype=torch.float32)
    with _timed('warp_perspective', detail=True, nbytes=4.0 * (x.numel() + out.numel())):
        _lib.call('mrefsr_warp_persp_f32', _p(x), _p(s), _p(out), n, c, h, w, ho, wo, WARP_INTERP[interp], int(clamp), _stream())
    return out


def match_stats(max_idx, M, thresholds=(1.0, 2.0), margin=0, valid_hw=None):
    """max_idx [N,h-2,w-2] int64 (the matcher's indices of N query / reference pairs) against the homographies M[n] (one 3 x 3 or N of
    them, float64) that map a query position to its true reference position in feature coordinates (views.to_feature_coords) ->
    [N, 2 + T] float64 on the device: per pair the number of counted queries, the sum of their end-point errors in feature pixels
    and, per threshold, the number of them with an error <= it.  A query counts if its top-left and its true target's both lie
    ``margin`` inside the valid map; valid_hw = (vh, vw) <= (h, w): the valid part of the feature maps (a zero-padded image),
    default the whole maps.  One launch, everything in double in a fixed order, nothing read back"""
    _chk('match_stats', max_idx, dtype=torch.int64)
    if max_idx.dim() != 3 or max_idx.numel() == 0:
        raise ValueError(f'match_stats: a non-empty [N,h-2,w-2] index tensor expected, got {tuple(max_idx.shape)}')
    n, h, w = max_idx.shape[0], max_idx.shape[1] + 2, max_idx.shape[2] + 2
    thr = [float(t) for t in thresholds]
    if len(thr) > MATCH_STATS_MAX_THRESHOLDS or any(not t >= 0 for t in thr):
        raise ValueError(f'match_stats: thresholds {thresholds!r}: at most {MATCH_STATS_MAX_THRESHOLDS} non-negative numbers expected')
    if isinstance(margin, bool) or not isinstance(margin, int) or margin < 0:
        raise ValueError(f'match_stats: margin {margin!r} is not a non-negative int')
    vh, vw = (h, w) if valid_hw is None else (int(v) for v in valid_hw)
    if not (3 <= vh <= h and 3 <= vw <= w):
        raise ValueError(f'match_stats: valid_hw ({vh}, {vw}) is not inside the {h} x {w} maps (3 <= vh <= h, 3 <= vw <= w)')
    m = _homographies('match_stats', M, n, max_idx.device)
    stats = torch.empty((n, 2 + len(thr)), device=max_idx.device, dtype=torch.float64)
    _lib.call('mrefsr_match_stats_f64', _p(max_idx), _p(m), (C.c_double * max(len(thr), 1))(*thr), _p(stats), n, h, w, vh - 3, vw - 3, margin,
              len(thr), _stream())
    return stats


def act_bwd_nhwc(g_out, out, act, slope=0.0, slope_ptr=None, want_bias=True, want_amax=False):
    """Backward of a fused convolution epilogue on [..., C] contiguous tensors: g_pre = g_out * act'(out) with act 0 none,
    1 LeakyReLU(slope) (0 = ReLU), 2 PReLU(slope_ptr).  Returns (g_pre [..., ld] with ld = C rounded up to 4 (extra channels
    zero: the dgrad convolution reads 16-byte channel vectors), bias gradient [C] | None, PReLU weight gradient [1] | None)."""
    _chk('act_bwd_nhwc', g_out, out, slope_ptr)
    c = g_out.shape[-1]
    npix = g_out.numel() // c
    blocks = _lib.load().mrefsr_act_bwd_blocks(npix, c)
    if blocks <= 0:
        raise ValueError(f'act_bwd_nhwc: unsupported channel count {c}')
    ld = (c + 3) // 4 * 4
    if act == 0 and ld == c:
        g_pre = None
        if not want_bias and not want_amax:
            return g_out, None, None
    elif ld == c:
        g_pre = torch.empty_like(g_out)
    else:
        g_pre = torch.zeros(g_out.shape[:-1] + (ld,), device=g_out.device, dtype=torch.float32)
    # the three zero-initialised accumulators of the kernel in ONE allocation (one fill launch instead of up to three)
    z = zeros_f32(g_out.device, c + 2) if (want_bias or act == 2 or want_amax) else None
    g_bias = z[:c] if want_bias else None
    g_slope = z[c:c + 1] if act == 2 else None
    amax = z[c + 1:c + 2] if want_amax else None
    flag = _p(_range_flag(g_out.device)) if act == 2 else None
    if (g_bias is not None or g_slope is not None) and is_deterministic():   # the sums added in block order (bitwise reproducible)
        need = blocks * (c + 1) * 4
        ws, ticket = _det_scratch(g_out.device, need)
        _lib.call('mrefsr_act_bwd_nhwc_det_f32', _p(g_out), _p(out if act else None), _p(g_pre), ld, _p(g_bias), _p(g_slope), _p(amax),
                  C.c_int64(npix), c, act, C.c_float(slope), _p(slope_ptr), flag, _p(ws), C.c_int64(need), _p(ticket), _stream())
    else:
        _lib.call('mrefsr_act_bwd_nhwc_f32', _p(g_out), _p(out if act else None), _p(g_pre), ld, _p(g_bias), _p(g_slope), _p(amax), C.c_int64(npix), c,
                  act, C.c_float(slope), _p(slope_ptr), flag, _stream())
    if want_amax:
        return (g_out if g_pre is None else g_pre), g_bias, g_slope, amax
    return (g_out if g_pre is None else g_pre), g_bias, g_slope


def conv_wgrad3x3(x, g, cin, cout, g_amax):
    """d loss / d weight [cout,cin,3,3] of a 3x3 'same' convolution from channels-last tensors x [N,H,W,>=cin], g [N,H,W,>=cout]
    (pixel-contiguous; extra trailing channels ignored); g_amax [1] = max |g| from act_bwd_nhwc(want_amax=True)"""
    n, h, w, _ = x.shape
    if tuple(g.shape[:3]) != (n, h, w):
        raise ValueError('conv_wgrad3x3: x / g sizes differ')
    ldx, ldg = _nhwc_ld('x', x), _nhwc_ld('g', g)
    _chk('conv_wgrad3x3', g_amax)
    dw = torch.empty((cout, cin, 3, 3), device=x.device, dtype=torch.float32)
    need = _lib.load().mrefsr_conv_wgrad3x3_workspace_bytes(n, h, w, cin, cout)
    ws = _scratch(x.device, need)
    _lib.call('mrefsr_conv_wgrad3x3_f32', _p(x), ldx, cin, _p(g), ldg, cout, _p(dw), C.c_int64(cin * 9), C.c_int64(9), 0, _p(g_amax), n, h, w,
              _p(ws), C.c_int64(need), _p(_range_flag(x.device)), _stream())
    return dw


def conv_wgrad3x3_batch(xs, gs, cin, cout, g_amaxes):
    """conv_wgrad3x3 for len(xs) <= 32 convolutions of one geometry in ONE launch pair (the convolutions of a residual trunk:
    their weight gradients feed nothing inside backward, so they can wait for each other); -> [n, cout, cin, 3, 3], row j = job j"""
    nj = len(xs)
    if not (0 < nj <= 32 and len(gs) == nj and len(g_amaxes) == nj):
        raise ValueError('conv_wgrad3x3_batch: 1..32 jobs, one g / g_amax per x')
    n, h, w, _ = xs[0].shape
    ldx, ldg = _nhwc_ld('x', xs[0]), _nhwc_ld('g', gs[0])
    for x, g in zip(xs, gs):
        if tuple(x.shape[:3]) != (n, h, w) or tuple(g.shape[:3]) != (n, h, w) or _nhwc_ld('x', x) != ldx or _nhwc_ld('g', g) != ldg:
            raise ValueError('conv_wgrad3x3_batch: the jobs of a batch share one geometry')
    _chk('conv_wgrad3x3_batch', *g_amaxes)
    dw = torch.empty((nj, cout, cin, 3, 3), device=xs[0].device, dtype=torch.float32)
    need = _lib.load().mrefsr_conv_wgrad3x3_batch_workspace_bytes(nj, n, h, w, cin, cout)
    ws = _scratch(xs[0].device, need)
    arr = C.c_void_p * nj
    _lib.call('mrefsr_conv_wgrad3x3_batch_f32', nj, arr(*[t.data_ptr() for t in xs]), ldx, cin, arr(*[t.data_ptr() for t in gs]), ldg, cout,
              arr(*[dw[j].data_ptr() for j in range(nj)]), C.c_int64(cin * 9), C.c_int64(9), 0, arr(*[t.data_ptr() for t in g_amaxes]), n, h, w,
              _p(ws), C.c_int64(need), _p(_range_flag(xs[0].device)), _stream())
    return dw


def mrattn_bwd_nhwc(q, emb, ass, g_out, t):
    """gradient of mrattn_fwd_nhwc: -> (g_q, g_emb, g_ass), same layouts"""
    _chk('mrattn_bwd_nhwc', q, emb, ass, g_out)
    n, h, w, c = q.shape
    if tuple(emb.shape) != (n * t, h, w, c) or tuple(ass.shape) != (n * t, h, w, 2 * c) or tuple(g_out.shape) != (n, h, w, 2 * c):
        raise ValueError('mrattn_bwd_nhwc: inconsistent shapes')
    g_q, g_emb, g_ass = torch.empty_like(q), torch.empty_like(emb), torch.empty_like(ass)
    _lib.call('mrefsr_mrattn_bwd_nhwc_f32', _p(q), _p(emb), _p(ass), _p(g_out), _p(g_q), _p(g_emb), _p(g_ass), n, t, c, h * w, _stream())
    return g_q, g_emb, g_ass


def mrattn_bwd_nhwc_masked(q, emb, ass, g_out, t, valid_bits, out=None):
    """gradient of mrattn_fwd_nhwc_masked: -> (g_q, g_emb, g_ass), same layouts; g_emb / g_ass of absent references are exact
    zeros.  out: the three buffers to write into (every element is written)"""
    _chk('mrattn_bwd_nhwc_masked', q, emb, ass, g_out)
    n, h, w, c = q.shape
    if tuple(emb.shape) != (n * t, h, w, c) or tuple(ass.shape) != (n * t, h, w, 2 * c) or tuple(g_out.shape) != (n, h, w, 2 * c):
        raise ValueError('mrattn_bwd_nhwc_masked: inconsistent shapes')
    _chk_valid_bits('mrattn_bwd_nhwc_masked', valid_bits, n)
    g_q, g_emb, g_ass = _grad_triple('mrattn_bwd_nhwc_masked', out, q, emb, ass)
    _lib.call('mrefsr_mrattn_bwd_nhwc_masked_f32', _p(q), _p(emb), _p(ass), _p(g_out), _p(valid_bits), _p(g_q), _p(g_emb), _p(g_ass), n, t, c,
              h * w, _stream())
    return g_q, g_emb, g_ass


def attn_modulate_bwd(g, refs, mul):
    """gradient of refs * sigmoid(mul) * 2 + add w.r.t. (refs, mul); d/d add = g"""
    _chk('attn_modulate_bwd', g, refs, mul)
    g_refs, g_mul = torch.empty_like(refs), torch.empty_like(mul)
    _lib.call('mrefsr_attn_modulate_bwd_f32', _p(g), _p(refs), _p(mul), _p(g_refs), _p(g_mul), C.c_int64(mul.numel()), _stream())
    return g_refs, g_mul


# ---- reflect pad / crop of channels-last maps (csrc/pad.hip): MRAPAFusion's pad to a multiple of 4 and crop back
def reflect_pad_nhwc(x, ph, pw):
    """x [N,H,W,C] -> [N,H+ph,W+pw,C], bottom / right reflect-padded (F.pad(mode='reflect') bit for bit); ph, pw in 0..3, < H, W"""
    _chk('reflect_pad_nhwc', x)
    n, h, w, c = x.shape
    out = torch.empty((n, h + ph, w + pw, c), device=x.device, dtype=torch.float32)
    with _timed('reflect_pad_nhwc', detail=True, nbytes=4.0 * (x.numel() + out.numel())):
        _lib.call('mrefsr_reflect_pad_nhwc_f32', _p(x), _p(out), n, h, w, c, ph, pw, _stream())
    return out


def reflect_pad_bwd_nhwc(g, ph, pw):
    """adjoint of reflect_pad_nhwc: g [N,H+ph,W+pw,C] -> [N,H,W,C] (mirrored contributions added in a fixed order)"""
    _chk('reflect_pad_bwd_nhwc', g)
    n, hp, wp, c = g.shape
    gx = torch.empty((n, hp - ph, wp - pw, c), device=g.device, dtype=torch.float32)
    with _timed('reflect_pad_bwd_nhwc', detail=True, nbytes=4.0 * (g.numel() + gx.numel())):
        _lib.call('mrefsr_reflect_pad_bwd_nhwc_f32', _p(g), _p(gx), n, hp - ph, wp - pw, c, ph, pw, _stream())
    return gx


def crop_nhwc(x, h0, w0, out_amax=None):
    """top-left h0 x w0 window of x [N,H,W,C] -> [N,h0,w0,C]; out_amax (a zeroed 1-element device word: amax_slot) receives max |out|"""
    _chk('crop_nhwc', x, out_amax)
    n, h, w, c = x.shape
    out = torch.empty((n, h0, w0, c), device=x.device, dtype=torch.float32)
    with _timed('crop_nhwc', detail=True, nbytes=8.0 * out.numel()):
        _lib.call('mrefsr_crop_nhwc_f32', _p(x), _p(out), _p(out_amax), n, h, w, c, h0, w0, _stream())
    return out


def crop_bwd_nhwc(g, h, w):
    """adjoint of crop_nhwc: g [N,h0,w0,C] -> [N,h,w,C], zero outside the window"""
    _chk('crop_bwd_nhwc', g)
    n, h0, w0, c = g.shape
    gx = torch.empty((n, h, w, c), device=g.device, dtype=torch.float32)
    with _timed('crop_bwd_nhwc', detail=True, nbytes=4.0 * (g.numel() + gx.numel())):
        _lib.call('mrefsr_crop_bwd_nhwc_f32', _p(g), _p(gx), n, h, w, c, h0, w0, _stream())
    return gx


# ---- max |out| words of the forward launches (mrefsr_conv_nhwc_amax_f32 / mrefsr_dcn_fwd_amax_f32): one zeroed float per producing
# launch, handed to the consumer as its in_amax.  A ring per device, two halves: a half is zeroed (one memset) when the slot counter
# enters it -- its words were handed out >= AMAX_POOL / 2 launches ago.  amax_pool_reset() (start of a pass:
# MultiRefRestorationModel.test / optimize_parameters) zeroes everything and restarts at slot 0, so that a captured graph re-zeroes
# and re-uses the same words in every replay.  Either event gives the words of a half to other launches: each half has a generation
# that moves with it, and the handle a word travels in (archs/nhwc.py) holds the generation it was issued in.
AMAX_POOL = 8192


class _AmaxRing:
    HALF = AMAX_POOL // 2

    def __init__(self, device):
        self.buf = torch.zeros(AMAX_POOL, device=device, dtype=torch.float32)
        self.views = list(self.buf.split(1))   # (the one-element views are made once: a slice per launch costs microseconds)
        self.next, self.gen = 0, [0, 0]

    def reset(self):
        self.buf.zero_()
        self.next, self.gen = 0, [g + 1 for g in self.gen]

    def slot(self):
        i = self.next % AMAX_POOL
        if i % self.HALF == 0:
            self.buf[i:i + self.HALF].zero_()
            self.gen[i // self.HALF] += 1
        self.next = i + 1
        return self.views[i]

    def generation(self, word):
        """of the half ``word`` (a slot()) lies in: it has moved once the word may be another launch's"""
        return self.gen[word.storage_offset() // self.HALF]

    @contextlib.contextmanager
    def one_half(self, option):
        """around a pass that takes words BEHIND those of a recorded forward, without a reset: a slot counter that wrapped, or ran
        into the ring's second half, would zero words in use -- the second half is what the backward pass may still take before the
        first one, which the recorded graph reads, is handed out again"""
        start = self.next
        yield
        used = self.next
        if used < start or used > self.HALF:
            raise RuntimeError(f'{option}: the forward and the EMA pass took {used} max |out| words (the pass from {start} on); a '
                               f'step has {self.HALF} of them, half of hip.AMAX_POOL = {AMAX_POOL}')


_amax_rings = {}


def amax_ring(device):
    return _amax_rings.get(device.index) or _amax_rings.setdefault(device.index, _AmaxRing(device))


def amax_pool_reset():
    for ring in _amax_rings.values():
        ring.reset()


def amax_slot(device):
    """a zeroed 1-element float32 device tensor for one launch's max |out|"""
    return amax_ring(device).slot()


def _nhwc_ld(name, t):
    """channel stride of a pixel for an [N,H,W,C] tensor that may be a channel slice of a wider one"""
    n, h, w, c = t.shape
    ld = t.stride(2)
    if not (t.is_cuda and t.dtype in (torch.float32, torch.bfloat16) and t.stride(3) == 1 and t.stride(1) == w * ld and t.stride(0) == h * w * ld):
        raise ValueError(f'conv_nhwc: {name} must be a pixel-contiguous float32 / bfloat16 NHWC device tensor, got shape '
                         f'{tuple(t.shape)} strides {t.stride()} dtype {t.dtype}')
    return ld


def conv_nhwc(x1, packed, bias, cout, ksize, x2=None, pre=None, residual=None, act=False, slope=0.0, slope_ptr=None,
              epilogue=0, out=None, terms=None, in_amax=None, out_amax=None):
    """Convolution (k = 1 / 3, stride 1, same padding) of cat([x1, x2], channel) with fused epilogue; all NHWC.

    x1 [N1,H,W,C1], x2 [N2,H,W,C2] (batch-broadcast: image n reads x[n % N]); pre [Np,H,W,cout] added
    before the activation (broadcast n % Np); act -> LeakyReLU(slope | *slope_ptr); residual [N,H,W,cout]
    added after it; epilogue 0 plain / 1 MaxPool2d(2,2) / 2 PixelShuffle(2).  `out` may be a channel
    slice of a wider NHWC buffer.  Returns out."""
    n1, h, w, c1 = x1.shape
    if terms is not None and terms != packed.terms:
        raise ValueError(f'conv_nhwc: weights packed for terms={packed.terms}, asked for terms={terms}')
    terms = packed.terms
    io16 = x1.dtype == torch.bfloat16
    if io16:
        if terms != 1:
            raise TypeError('conv_nhwc: bfloat16 tensors go with the bf16 arithmetic (weights packed with terms=1)')
        for t_ in (x2, pre, residual, out):
            if t_ is not None and t_.dtype != torch.bfloat16:
                raise TypeError('conv_nhwc: with a bfloat16 x1 every activation tensor must be bfloat16')
        terms = 2   # descriptor code of "terms = 1 arithmetic on bf16 tensors"
    d = _lib.ConvDesc()
    d.wscale = packed.wscale
    d.H, d.W, d.ksize, d.C1, d.ld1, d.N1 = h, w, ksize, c1, _nhwc_ld('x1', x1), n1
    n = n1
    if x2 is not None:
        d.C2, d.ld2, d.N2 = x2.shape[3], _nhwc_ld('x2', x2), x2.shape[0]
        if tuple(x2.shape[1:3]) != (h, w):
            raise ValueError('conv_nhwc: x1 / x2 spatial size mismatch')
        n = max(n, x2.shape[0])
    if residual is not None:
        n = max(n, residual.shape[0])
        d.ld_res = _nhwc_ld('residual', residual)
    if pre is not None:
        _chk('conv_nhwc', pre, dtype=x1.dtype)
        d.pre_N = pre.shape[0]
    d.N, d.Cout, d.act, d.epilogue, d.terms, d.slope = n, cout, 1 if act else 0, epilogue, terms, slope
    oshape = {0: (n, h, w, cout), 1: (n, h // 2, w // 2, cout), 2: (n, 2 * h, 2 * w, cout // 4)}[epilogue]
    if out is None:
        out = torch.empty(oshape, device=x1.device, dtype=x1.dtype)
    elif tuple(out.shape) != oshape:
        raise ValueError(f'conv_nhwc: out shape {tuple(out.shape)} != {oshape}')
    d.ld_out = _nhwc_ld('out', out)
    _chk('conv_nhwc', bias, slope_ptr)
    es = x1.element_size()   # algorithmic bytes of the launch: every operand and the result once (broadcast operands once)
    nby = (x1.numel() + (x2.numel() if x2 is not None else 0) + (pre.numel() if pre is not None else 0) +
           (residual.numel() if residual is not None else 0) + out.shape[0] * out.shape[1] * out.shape[2] * oshape[3]) * es + \
        4.0 * (d.C1 + d.C2) * cout * ksize * ksize
    with _timed('conv_wino_k3' if terms == 17 else f'conv_nhwc_k{ksize}', 2.0 * n * h * w * (d.C1 + d.C2) * cout * ksize * ksize, detail=True, nbytes=nby):
        if out_amax is not None:   # + max |out| into out_amax[0] (a zeroed device word: amax_slot): the next Winograd layer's input scale
            _chk('conv_nhwc', in_amax, out_amax)
            _lib.call('mrefsr_conv_nhwc_amax_f32', C.byref(d), _p(x1), _p(x2), _p(packed.data), _p(bias), _p(slope_ptr), _p(pre),
                      _p(residual), _p(out), _p(_range_flag(x1.device)), _p(in_amax), _p(out_amax), _stream())
        elif in_amax is not None:   # inputs of unknown magnitude (gradients): scaled into the fp16 range by the kernel, terms 16 only
            _lib.call('mrefsr_conv_nhwc_scaled_f32', C.byref(d), _p(x1), _p(x2), _p(packed.data), _p(bias), _p(slope_ptr), _p(pre),
                      _p(residual), _p(out), _p(_range_flag(x1.device)), _p(in_amax), _stream())
        else:
            _lib.call('mrefsr_conv_nhwc_f32', C.byref(d), _p(x1), _p(x2), _p(packed.data), _p(bias), _p(slope_ptr), _p(pre), _p(residual),
                      _p(out), _p(_range_flag(x1.device) if terms in (16, 17) else None), _stream())
    return out


def conv_nhwc_bwd(x, packed, cout, ksize, residual=None, residual_is_mask=False, in_amax=None, want_stats=True):
    """Input-gradient convolution of a training step with the pass that would follow it folded in (mrefsr_conv_nhwc_bwd_f32):
    out = conv(x) + residual, or conv(x) where residual > 0 (``residual_is_mask``: the ReLU of the layer below); with
    ``want_stats`` also the per-channel sums of out (a bias gradient) and max |out| (the fp16 input scale of whatever reads out
    next).  terms-16 packed weights, fp32 channels-last tensors.  -> (out, sums [cout] | None, amax [1] | None)"""
    if packed.terms != 16:
        raise ValueError('conv_nhwc_bwd: weights packed with terms=16 expected')
    n, h, w, c1 = x.shape
    d = _lib.ConvDesc()
    d.wscale = packed.wscale
    d.N, d.H, d.W, d.ksize, d.C1, d.ld1, d.N1 = n, h, w, ksize, c1, _nhwc_ld('x', x), n
    d.Cout, d.act, d.epilogue, d.terms, d.slope = cout, 0, 0, 16, 0.0
    if residual is not None:
        if tuple(residual.shape) != (n, h, w, cout):
            raise ValueError('conv_nhwc_bwd: residual / mask source must have the output shape')
        d.ld_res = _nhwc_ld('residual', residual)
    out = torch.empty((n, h, w, cout), device=x.device, dtype=torch.float32)
    d.ld_out = cout
    _chk('conv_nhwc_bwd', x, residual, in_amax)
    z = zeros_f32(x.device, cout + 1) if want_stats else None
    if want_stats and is_deterministic():   # the per-cout sums added in tile order (bitwise reproducible)
        need = _lib.load().mrefsr_conv_nhwc_bwd_det_workspace_bytes(C.byref(d))
        ws, ticket = _det_scratch(x.device, need)
        _lib.call('mrefsr_conv_nhwc_bwd_det_f32', C.byref(d), _p(x), _p(packed.data), _p(residual), 1 if residual_is_mask else 0, _p(out),
                  _p(_range_flag(x.device)), _p(in_amax), _p(z[:cout]), _p(z[cout:]), _p(ws), C.c_int64(need), _p(ticket), _stream())
        return out, z[:cout], z[cout:]
    _lib.call('mrefsr_conv_nhwc_bwd_f32', C.byref(d), _p(x), _p(packed.data), _p(residual), 1 if residual_is_mask else 0, _p(out),
              _p(_range_flag(x.device)), _p(in_amax), _p(z[:cout]) if want_stats else None, _p(z[cout:]) if want_stats else None, _stream())
    return out, (z[:cout] if want_stats else None), (z[cout:] if want_stats else None)


def conv_dynagg(x, packed, bias, pre, dg, abs_sum=None):
    """conv_offset_mask (3x3, C -> 27 dg) of a DynAgg with the glue of ref :56-73 as its epilogue: x [N,H,W,C] channels-last
    -> planar (offset [N,18dg,H,W], mask [N,9dg,H,W]) for dcn_fwd; pre [N,9,H,W,2] ([x,y]); abs_sum float64[1] or None"""
    n, h, w, c = x.shape
    _chk('conv_dynagg', pre, bias)
    if tuple(pre.shape) != (n, 9, h, w, 2):
        raise ValueError(f'conv_dynagg: pre {tuple(pre.shape)} does not match x {tuple(x.shape)}')
    if abs_sum is not None:
        _chk('conv_dynagg', abs_sum, dtype=torch.float64)
    d = _lib.ConvDesc()
    d.wscale, d.terms = packed.wscale, (2 if (x.dtype == torch.bfloat16 and packed.terms == 1) else packed.terms)
    d.N, d.H, d.W, d.ksize, d.C1, d.ld1, d.N1, d.Cout = n, h, w, 3, c, _nhwc_ld('x', x), n, 27 * dg
    offset = torch.empty((n, 18 * dg, h, w), device=x.device, dtype=torch.float32)
    mask = torch.empty((n, 9 * dg, h, w), device=x.device, dtype=torch.float32)
    nby = x.numel() * x.element_size() + (pre.numel() + offset.numel() + mask.numel()) * 4.0 + 4.0 * c * 27 * dg * 9
    with _timed('conv_nhwc_k3', 2.0 * n * h * w * c * 27 * dg * 9, detail=True, nbytes=nby):
        _lib.call('mrefsr_conv_dynagg_f32', C.byref(d), _p(x), _p(packed.data), _p(bias), _p(pre), _p(offset), _p(mask), _p(abs_sum), dg,
                  _p(_range_flag(x.device) if packed.terms == 16 else None), _stream())
    return offset, mask


def image_to_nhwc4(img, mean=None, std=None, range_norm=False):
    """[N,3,H,W] float32 (contiguous) -> [N,H,W,4]: ((img + 1) / 2 if range_norm) then ((. - mean) / std if mean is given; 3-element
    device tensors) in channels 0..2, zero in channel 3 -- the extractors' input normalisation and channels-last packing in one pass"""
    _chk('image_to_nhwc4', img, mean, std)
    n, c, h, w = img.shape
    if c != 3:
        raise ValueError(f'image_to_nhwc4: 3 channels expected, got {c}')
    if mean is not None and (mean.numel() != 3 or std is None or std.numel() != 3):
        raise ValueError('image_to_nhwc4: mean / std must hold 3 values each')
    out = torch.empty((n, h, w, 4), device=img.device, dtype=torch.float32)
    _lib.call('mrefsr_image_to_nhwc4_f32', _p(img), _p(out), C.c_int64(n), C.c_int64(h * w), 1 if range_norm else 0, _p(mean), _p(std), _stream())
    return out


def attn_modulate_(refs, mul, add=None):
    """mul <- refs * sigmoid(mul) * 2 + add, in place on ``mul`` (all three contiguous, same shape); fp32 with ``add`` None: the same
    without the last add (the addend travels as the `pre` of feat_fusion's launch)"""
    b16 = mul.dtype == torch.bfloat16
    _chk('attn_modulate', refs, mul, add, dtype=mul.dtype if b16 else torch.float32)
    if refs.shape != mul.shape or (add is not None and add.shape != mul.shape):
        raise ValueError('attn_modulate: shape mismatch')
    if add is None and b16:
        raise NotImplementedError('attn_modulate: the bf16 arithmetic keeps its addend (its rounding points are fixed)')
    _lib.call('mrefsr_attn_modulate_bf16' if b16 else 'mrefsr_attn_modulate_f32', _p(refs), _p(mul), _p(add), C.c_int64(mul.numel()), _stream())
    return mul


def bias_relu_pool2(x, bias):
    """x [N,C,H,W] (conv output without bias) -> relu(maxpool2x2(x) + bias) [N,C,H/2,W/2]"""
    _chk('bias_relu_pool2', x, bias)
    n, c, h, w = x.shape
    out = torch.empty((n, c, h // 2, w // 2), device=x.device, dtype=torch.float32)
    _lib.call('mrefsr_bias_relu_pool2_f32', _p(x), _p(bias), _p(out), C.c_int64(n), c, h, w, _stream())
    return out


def upfirdn2d(x, kernel, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1):
    """x [major,in_h,in_w,minor] -> [major,out_h,out_w,minor]  (upfirdn2d.cpp:13-24)."""
    if x.dtype not in _DT:
        raise TypeError(f'upfirdn2d: unsupported dtype {x.dtype}')
    x, kernel = x.contiguous(), kernel.to(x.dtype).contiguous()
    _chk('upfirdn2d', x, kernel, dtype=x.dtype)
    mj, ih, iw, mn = x.shape
    kh, kw = kernel.shape
    oh = (ih * up_y + pad_y0 + pad_y1 - kh + down_y) // down_y
    ow = (iw * up_x + pad_x0 + pad_x1 - kw + down_x) // down_x
    out = torch.empty((mj, oh, ow, mn), device=x.device, dtype=x.dtype)
    _lib.call('mrefsr_upfirdn2d', _p(x), _p(kernel), _p(out), mj, ih, iw, mn, kh, kw, up_x, up_y, down_x, down_y,
              pad_x0, pad_x1, pad_y0, pad_y1, _DT[x.dtype], _stream())
    return out


# ------------------------------------------------------------------ perceptual / style loss (csrc/percep.hip)
def maxpool2_nhwc(x, relu=False, want_plane=False):
    """MaxPool2d(2, 2) of [N,H,W,C] (C % 4 == 0; floor sizes, torch's tie rule); relu: pools max(x, 0).  -> (out [N,H//2,W//2,C],
    plane uint8 [N,H//2,W//2,C] | None: bits 0-1 arg-max, bit 2 max > 0)"""
    _chk('maxpool2_nhwc', x)
    n, h, w, c = x.shape
    out = torch.empty((n, h // 2, w // 2, c), device=x.device, dtype=torch.float32)
    plane = torch.empty((n, h // 2, w // 2, c), device=x.device, dtype=torch.uint8) if want_plane else None
    with _timed('maxpool2_nhwc', detail=True, nbytes=4.0 * (x.numel() + out.numel())):
        _lib.call('mrefsr_maxpool2_nhwc_f32', _p(x), _p(out), _p(plane), n, h, w, c, 1 if relu else 0, _stream())
    return out, plane


def maxpool2_bwd_nhwc(g, x=None, plane=None, relu=False, mask=True, shape=None, want_amax=True):
    """gradient of [ReLU ->] MaxPool2d(2, 2): g [N,H//2,W//2,C] -> (g_in [N,H,W,C], max |g_in| [1] | None).  The arg-max comes from
    `plane` (maxpool2_nhwc(want_plane=True)) or is recomputed from the pre-pool map x; mask: times the ReLU derivative.
    shape = (N, H, W, C) when only the plane is given."""
    _chk('maxpool2_bwd_nhwc', g, x)
    if plane is not None and (plane.dtype != torch.uint8 or not plane.is_contiguous() or tuple(plane.shape) != tuple(g.shape)):
        raise ValueError('maxpool2_bwd_nhwc: plane must be a contiguous uint8 tensor of the pooled shape')
    n, h, w, c = tuple(x.shape) if x is not None else tuple(shape)
    if tuple(g.shape) != (n, h // 2, w // 2, c):
        raise ValueError(f'maxpool2_bwd_nhwc: g {tuple(g.shape)} is not the pooled shape of {(n, h, w, c)}')
    g_in = torch.empty((n, h, w, c), device=g.device, dtype=torch.float32)
    amax = zeros_f32(g.device, 1) if want_amax else None
    with _timed('maxpool2_bwd_nhwc', detail=True, nbytes=4.0 * (g.numel() + g_in.numel() + (x.numel() if plane is None else g.numel() / 4))):
        _lib.call('mrefsr_maxpool2_bwd_nhwc_f32', _p(g), _p(x), _p(plane), _p(g_in), _p(amax), n, h, w, c, 1 if relu else 0,
                  1 if mask else 0, _stream())
    return g_in, amax


CRIT = {'l1': 0, 'fro': 1}


def _tap_jobs(xs, ys, weights, groups, grads=None):
    import numpy as np
    jobs = (_lib.TapJob * len(xs))()
    for j, (x, y) in enumerate(zip(xs, ys)):
        _chk('tap_crit', x, y)
        if x.shape != y.shape:
            raise ValueError('tap_crit: x / y shapes differ')
        g = grads[j] if grads is not None else None
        if g is not None:
            _chk('tap_crit', g)
            if g.shape != x.shape:
                raise ValueError('tap_crit: grad must have the shape of x')
        n = x.numel()
        jobs[j] = _lib.TapJob(x.data_ptr(), y.data_ptr(), 0 if g is None else g.data_ptr(), n, float(np.float32(1.0) / np.float32(n)),
                              float(weights[j]), int(groups[j]))
    return jobs


def tap_crit_loss(xs, ys, weights, groups, crit, loss_weights):
    """criterion of several taps in one launch pair, fixed summation order: -> (losses [J] = l1 mean |x - y| or fro ||x - y||,
    totals [2] = (sum_j losses[j] * weights[j] over group g) * loss_weights[g])"""
    jobs = _tap_jobs(xs, ys, weights, groups)
    lib = _lib.load()
    nb = lib.mrefsr_tap_crit_workspace_bytes(jobs, len(xs))
    dev = xs[0].device
    part = torch.empty(nb // 8, device=dev, dtype=torch.float64)
    losses = torch.empty(len(xs), device=dev, dtype=torch.float32)
    totals = torch.empty(2, device=dev, dtype=torch.float32)
    with _timed('tap_crit', detail=True, nbytes=8.0 * sum(x.numel() for x in xs)):
        _lib.call('mrefsr_tap_crit_f32', jobs, len(xs), CRIT[crit], C.c_float(loss_weights[0]), C.c_float(loss_weights[1]), None, None, 0,
                  _p(part), _p(losses), _p(totals), None, _stream())
    return losses, totals


def tap_crit_grad(x, y, grad, weight, group, crit, loss_weights, gup=None, norm=None, accumulate=False, want_amax=True):
    """grad (+)= d total / d x of one tap (torch's autograd arithmetic, times gup[group] -- a device tensor [2] or None = 1); norm:
    the tap's Frobenius norm from tap_crit_loss (crit 'fro').  -> max |grad| [1] | None"""
    jobs = _tap_jobs([x], [y], [weight], [group], [grad])
    if gup is not None:
        _chk('tap_crit', gup)
    if crit == 'fro':
        _chk('tap_crit', norm)
    amax = zeros_f32(x.device, 1) if want_amax else None
    with _timed('tap_crit', detail=True, nbytes=4.0 * x.numel() * (4 if accumulate else 3)):
        _lib.call('mrefsr_tap_crit_f32', jobs, 1, CRIT[crit], C.c_float(loss_weights[0]), C.c_float(loss_weights[1]), _p(gup),
                  _p(norm) if crit == 'fro' else None, 1 if accumulate else 0, None, None, None, _p(amax), _stream())
    return amax


def _gram(name, f, scale):
    """f [N,H,W,C] -> [N,C,C] = F^T F * scale per image; scale None: 1 / (C H W), which the library forms in fp32"""
    _chk(name, f)
    n, h, w, c = f.shape
    need = _lib.load().mrefsr_gram_workspace_bytes(n, h * w, c)
    if need < 0:
        raise ValueError(f'{name}: C={c} (a multiple of 64)')
    ws = _scratch(f.device, need)
    g = torch.empty((n, c, c), device=f.device, dtype=torch.float32)
    with _timed('gram_nhwc', 2.0 * n * h * w * c * c, detail=True, nbytes=4.0 * (f.numel() + g.numel())):
        if scale is None:
            _lib.call('mrefsr_gram_nhwc_f32', _p(f), n, h * w, c, _p(g), _p(ws), C.c_int64(need), _stream())
        else:
            _lib.call('mrefsr_gram_nhwc_scaled_f32', _p(f), n, h * w, c, C.c_float(scale), _p(g), _p(ws), C.c_int64(need), _stream())
    return g


def gram_nhwc(f):
    """f [N,H,W,C] (C a multiple of 64) -> [N,C,C] = F^T F / (C H W) per image (exact f32 MFMA products, fixed summation order)"""
    return _gram('gram_nhwc', f, None)


def _gram_bwd_shapes(name, f, gx, gy, df):
    """the shapes gram_bwd_nhwc and texture_gram_bwd_nhwc share: f, df [N,H,W,C]; gx, gy [N,C,C] -> (n, h, w, c)"""
    n, h, w, c = f.shape
    if tuple(gx.shape) != (n, c, c) or tuple(gy.shape) != (n, c, c) or tuple(df.shape) != tuple(f.shape):
        raise ValueError(f'{name}: inconsistent shapes')
    return n, h, w, c


def gram_bwd_nhwc(f, gx, gg, df, loss_weight, weight, gup=None, accumulate=False, want_amax=True):
    """df [N,H,W,C] (+)= d style / d f of the l1 style term  ((l1(gram(f), gg) * weight) * loss_weight) * gup: (2 / (C H W)) F S,
    S = sgn(gx - gg) * ((gup * loss_weight) * weight) / (N C C); gx = gram_nhwc(f).  gup: a device scalar or None (= 1).
    -> max |df| [1] | None"""
    _chk('gram_bwd_nhwc', f, gx, gg, df, gup)
    n, h, w, c = _gram_bwd_shapes('gram_bwd_nhwc', f, gx, gg, df)
    amax = zeros_f32(f.device, 1) if want_amax else None
    with _timed('gram_bwd_nhwc', 2.0 * n * h * w * c * c, detail=True, nbytes=4.0 * (2 + accumulate) * f.numel()):
        _lib.call('mrefsr_gram_bwd_nhwc_f32', _p(f), _p(gx), _p(gg), _p(df), n, h * w, c, _p(gup), C.c_float(loss_weight), C.c_float(weight),
                  1 if accumulate else 0, _p(amax), _stream())
    return amax


# ------------------------------------------------------------------ texture loss and its swapped maps (csrc/texture.hip)
def texture_select(idx, val, valid_bits=None):
    """idx int64, val fp32 [K,B,gh,gw] (the matcher's outputs, k-major) -> (sel int32 [B,gh,gw]: the present reference with the
    largest val, the lowest k among equal ones; weights fp32 [B,1,gh,gw]: that value; pidx int32 [B,gh,gw]: idx[sel]).
    valid_bits: int32 [B], bit k = reference k of the sample is present (None: all)."""
    _chk('texture_select', idx, dtype=torch.int64)
    _chk('texture_select', val)
    if idx.dim() != 4 or idx.shape != val.shape or idx.shape[0] > 32:
        raise ValueError(f'texture_select: idx / val must be [K,B,gh,gw] with K <= 32, got {tuple(idx.shape)} / {tuple(val.shape)}')
    k, b, gh, gw = idx.shape
    if valid_bits is not None:
        _chk_valid_bits('texture_select', valid_bits, b)
    sel = torch.empty((b, gh, gw), device=idx.device, dtype=torch.int32)
    pidx = torch.empty_like(sel)
    wts = torch.empty((b, 1, gh, gw), device=idx.device, dtype=torch.float32)
    with _timed('texture_select', detail=True, nbytes=12.0 * idx.numel() + 12.0 * sel.numel()):
        _lib.call('mrefsr_texture_select_f32', _p(idx), _p(val), _p(valid_bits), _p(sel), _p(wts), _p(pidx), k, b, C.c_int64(gh * gw), _stream())
    return sel, wts, pidx


# ------------------------------------------------------------------ reference pools: the K best of N candidates (csrc/refselect.hip)
REF_SCORE_MODES = {'mean': 0, 'wins': 1}   # MREFSR_REF_SCORE_MEAN / _WINS


def ref_select(val, valid_bits, k, score='mean'):
    """val fp32 [N,B,gh,gw] (or [N,B,P]): the matcher's winning correlations of the N candidates (candidate-major);
    valid_bits int32 [B] on the device, bit n = candidate n of the sample is present (None: all) -> (sel int32 [B,k]: per sample the
    min(k, present) best candidates by (score descending, n ascending), written in ascending n, -1 behind them; slot_bits int32 [B]:
    one bit per filled slot; scores fp32 [B,N], -inf for absent candidates).  score 'mean': the fp32 mean of val over the positions
    in a fixed order that depends on P alone; 'wins': the number of positions the candidate wins (texture_select's rule).  Two
    launches, no readback."""
    if score not in REF_SCORE_MODES:
        raise ValueError(f"ref_select: score {score!r} is not 'mean' or 'wins'")
    _chk('ref_select', val)
    if val.dim() not in (3, 4) or val.numel() == 0 or val.shape[0] > 32:
        raise ValueError(f'ref_select: val must be a non-empty [N,B,gh,gw] or [N,B,P] tensor with N <= 32, got {tuple(val.shape)}')
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 32:
        raise ValueError(f'ref_select: k {k!r} is not an int in 1..32')
    n, b = val.shape[:2]
    p = val[0, 0].numel()
    if valid_bits is not None:
        _chk_valid_bits('ref_select', valid_bits, b)
    sel = torch.empty((b, k), device=val.device, dtype=torch.int32)
    slot_bits = torch.empty((b,), device=val.device, dtype=torch.int32)
    scores = torch.empty((b, n), device=val.device, dtype=torch.float32)
    ws_bytes = _lib.load().mrefsr_ref_select_workspace_bytes(n, b, p)
    ws = torch.empty(max(ws_bytes, 4) // 4, device=val.device, dtype=torch.int32)
    with _timed('ref_select', detail=True, nbytes=4.0 * val.numel()):
        _lib.call('mrefsr_ref_select_f32', _p(val), _p(valid_bits), _p(scores), _p(sel), _p(slot_bits), n, b, C.c_int64(p), k,
                  REF_SCORE_MODES[score], _p(ws), C.c_int64(ws_bytes), _stream())
    return sel, slot_bits, scores


def ref_gather(src, sel, n, out=None):
    """src [n*B, ...] (contiguous fp32 or int64, candidate-major), sel int32 [B,K] from ref_select -> [K*B, ...] (slot-major):
    row k*B + b = src row sel[b,k]*B + b, zeros where sel[b,k] is -1.  A new tensor (not an engine product: no cached max |out|
    travels with it), or ``out`` (its first K*B rows are written, nothing else).  One launch."""
    if src.dtype not in (torch.float32, torch.int64):
        raise TypeError(f'ref_gather: float32 or int64 rows expected, got {src.dtype}')
    _chk('ref_gather', src, dtype=src.dtype)
    _chk('ref_gather', sel, dtype=torch.int32)
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= 32 or src.dim() < 2 or src.numel() == 0 or src.shape[0] % n:
        raise ValueError(f'ref_gather: a non-empty [n*B, ...] tensor with n in 1..32 expected, got {tuple(src.shape)} with n = {n!r}')
    b = src.shape[0] // n
    if sel.dim() != 2 or sel.shape[0] != b or not 1 <= sel.shape[1] <= 32:
        raise ValueError(f'ref_gather: sel must be [{b}, K] with K in 1..32, got {tuple(sel.shape)}')
    k = sel.shape[1]
    if out is None:
        out = torch.empty((k * b, *src.shape[1:]), device=src.device, dtype=src.dtype)
    else:
        _chk('ref_gather', out, dtype=src.dtype)
        if out.dim() != src.dim() or out.shape[0] < k * b or out.shape[1:] != src.shape[1:]:
            raise ValueError(f'ref_gather: out {tuple(out.shape)} does not hold {k * b} rows of {tuple(src.shape[1:])}')
    row_bytes = src[0].numel() * src.element_size()
    with _timed('ref_gather', detail=True, nbytes=2.0 * k * b * row_bytes):
        _lib.call('mrefsr_ref_gather', _p(src), _p(out), _p(sel), n, b, k, C.c_int64(row_bytes), _stream())
    return out


# ------------------------------------------------------------------ SSIM loss of the training step (csrc/ssim_loss.hip)
SSIM_TILE = (16, 32)   # map positions per forward block / pixels per backward block (rows, columns)


def _ssim_planes(name, shape, rgb):
    """(B, H, W, planes) of a [B,3,H,W] call of the SSIM and MS-SSIM kernels: one plane per image, three with rgb, or ValueError"""
    if len(shape) != 4 or shape[1] != 3:
        raise ValueError(f'{name}: [B,3,H,W] images expected, got {tuple(shape)}')
    b, _, h, w = shape
    return b, h, w, (3 if rgb else 1) * b


def _ssim_shape(name, pred, target, rgb):
    _chk(name, pred, target)
    if pred.shape != target.shape:
        raise ValueError(f'{name}: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ')
    b, h, w, planes = _ssim_planes(name, pred.shape, rgb)
    blocks = _lib.load().mrefsr_ssim_loss_blocks(b, h, w, int(bool(rgb)))
    if blocks <= 0:
        raise ValueError(f'{name}: unsupported shape {tuple(pred.shape)} (B <= 21845, 11 <= H, W <= 2^19, H W <= 2^30)')
    return b, h, w, planes, blocks


def ssim_loss_fwd(pred, target, rgb=False, loss_weight=1.0, want_grad=False):
    """pred, target [B,3,H,W] (contiguous fp32) -> (loss, maps): loss a 0-dim tensor = loss_weight (1 - mean SSIM map) over the Y
    plane of every image (rgb=False) or its three colour planes at 255 scale (rgb=True); maps: None, or with want_grad the
    coefficient maps (a, b, c), each [planes,H-10,W-10], that ssim_loss_bwd reads.  One launch, a fixed summation order (the same
    bits from call to call), nothing read back; pred and target are only read"""
    b, h, w, planes, blocks = _ssim_shape('ssim_loss_fwd', pred, target, rgb)
    maps = tuple(torch.empty((planes, h - 10, w - 10), device=pred.device, dtype=torch.float32) for _ in range(3)) if want_grad else None
    loss = torch.empty((), device=pred.device, dtype=torch.float32)
    part, ticket = _det_scratch(pred.device, 4 * blocks)
    a, bb, c = maps if want_grad else (None, None, None)
    with _timed('ssim_loss_fwd', detail=True, nbytes=4.0 * (2 * pred.numel() + (3 * planes * (h - 10) * (w - 10) if want_grad else 0))):
        _lib.call('mrefsr_ssim_loss_fwd_f32', _p(pred), _p(target), b, h, w, int(bool(rgb)), C.c_float(loss_weight), _p(a), _p(bb), _p(c),
                  _p(part), _p(ticket), _p(loss), _stream())
    return loss, maps


def ssim_loss_bwd(pred, target, maps, grad_loss, rgb=False, loss_weight=1.0):
    """d (grad_loss * loss) / d pred [B,3,H,W] of ssim_loss_fwd from its coefficient maps; grad_loss: the upstream gradient, a
    one-element fp32 device tensor (read by the kernel, not by the host).  One launch; every element is written once"""
    b, h, w, planes, _ = _ssim_shape('ssim_loss_bwd', pred, target, rgb)
    _chk('ssim_loss_bwd', grad_loss, *maps)
    if grad_loss.numel() != 1 or len(maps) != 3 or any(m.shape != (planes, h - 10, w - 10) for m in maps):
        raise ValueError(f'ssim_loss_bwd: one upstream value and three maps of {(planes, h - 10, w - 10)} expected')
    grad = torch.empty_like(pred)
    with _timed('ssim_loss_bwd', detail=True, nbytes=4.0 * (3 * pred.numel() + 3 * maps[0].numel())):
        _lib.call('mrefsr_ssim_loss_bwd_f32', _p(pred), _p(target), _p(maps[0]), _p(maps[1]), _p(maps[2]), _p(grad_loss), b, h, w,
                  int(bool(rgb)), C.c_float(loss_weight), _p(grad), _stream())
    return grad


# ------------------------------------------------------------------ multi-scale SSIM: loss and validation metric (csrc/msssim.hip)
MSSSIM_MAX_LEVELS = 5   # MREFSR_MSSSIM_MAX_LEVELS (losses.py takes it from here)


def _msssim_shape(name, shape, rgb, levels):
    """(B, H, W, planes, floats of the two pyramids, floats of the three map sets) of a [B,3,H,W] call, or ValueError"""
    b, h, w, planes = _ssim_planes(name, shape, rgb)
    lib = _lib.load()
    pyr = lib.mrefsr_msssim_pyramid_floats(b, h, w, int(bool(rgb)), int(levels))
    if pyr <= 0:
        raise ValueError(f'{name}: unsupported shape {tuple(shape)} with {levels} levels (1..{MSSSIM_MAX_LEVELS} levels, '
                         'min(H, W) >> (levels - 1) >= 11, B <= 21845, H, W <= 2^19, H W <= 2^30)')
    return b, h, w, planes, pyr, lib.mrefsr_msssim_map_floats(b, h, w, int(bool(rgb)), int(levels))


def msssim_loss_fwd(pred, target, weights, rgb=False, loss_weight=1.0, want_grad=False, want_values=False):
    """pred, target [B,3,H,W] (contiguous fp32) -> (loss, saved, values): loss a 0-dim tensor = loss_weight (1 - mean_p v_p), v_p the
    MS-SSIM of plane p (Y plane of every image, or with rgb=True its three colour planes at 255 scale) over len(weights) levels
    with the weights used as given;
    saved: None, or with want_grad (pyramid, maps, mult), what msssim_loss_bwd reads; values: None, or with want_values v_p
    [planes] in float64.  Three launches, a fixed summation order (the same bits from call to call), nothing read back; pred and
    target are only read"""
    _chk('msssim_loss_fwd', pred, target)
    if pred.shape != target.shape:
        raise ValueError(f'msssim_loss_fwd: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ')
    levels = len(weights)
    b, h, w, planes, pyr_floats, map_floats = _msssim_shape('msssim_loss_fwd', pred.shape, rgb, levels)
    dev = pred.device
    ws_bytes = _lib.load().mrefsr_msssim_workspace_bytes(b, h, w, int(bool(rgb)), levels, 0)
    loss = torch.empty((), device=dev, dtype=torch.float32)
    values = torch.empty(planes, device=dev, dtype=torch.float64) if want_values else None
    if want_grad:     # what the backward reads outlives this call: tensors of its own, not scratch
        pyramid = torch.empty(pyr_floats, device=dev, dtype=torch.float32)
        maps = torch.empty(map_floats, device=dev, dtype=torch.float32)
        mult = torch.empty((planes, levels), device=dev, dtype=torch.float32)
        ws = _scratch(dev, ws_bytes)
    else:
        maps = mult = None
        pyr_bytes = (4 * pyr_floats + 255) // 256 * 256
        buf = _scratch(dev, pyr_bytes + ws_bytes)
        pyramid, ws = buf, buf[pyr_bytes:]
    wts = (C.c_double * MSSSIM_MAX_LEVELS)(*[float(v) for v in weights])
    with _timed('msssim_loss_fwd', detail=True, nbytes=4.0 * (2 * pred.numel() + 2 * pyr_floats + (map_floats if want_grad else 0))):
        _lib.call('mrefsr_msssim_loss_fwd_f32', _p(pred), _p(target), b, h, w, int(bool(rgb)), levels, wts, C.c_float(loss_weight),
                  _p(pyramid), _p(maps), _p(mult), _p(values), _p(ws), C.c_int64(ws_bytes), _p(loss), _stream())
    return loss, ((pyramid, maps, mult) if want_grad else None), values


def msssim_loss_bwd(saved, grad_loss, shape, rgb=False, loss_weight=1.0):
    """d (grad_loss * loss) / d pred [B,3,H,W] (= shape) of msssim_loss_fwd from what it saved; grad_loss: the upstream gradient, a
    one-element fp32 device tensor (read by the kernels, not by the host).  Two launches (one for a single level); every element is
    written once"""
    pyramid, maps, mult = saved
    _chk('msssim_loss_bwd', grad_loss, pyramid, maps, mult)
    levels = mult.shape[1] if mult.dim() == 2 else 0
    b, h, w, planes, pyr_floats, map_floats = _msssim_shape('msssim_loss_bwd', shape, rgb, levels)
    if grad_loss.numel() != 1 or pyramid.numel() != pyr_floats or maps.numel() != map_floats or mult.shape[0] != planes:
        raise ValueError(f'msssim_loss_bwd: one upstream value, a pyramid of {pyr_floats}, maps of {map_floats} floats and multipliers '
                         f'[{planes}, {levels}] expected')
    ws_bytes = _lib.load().mrefsr_msssim_workspace_bytes(b, h, w, int(bool(rgb)), levels, 1)
    ws = _scratch(pyramid.device, ws_bytes) if ws_bytes else None
    grad = torch.empty(tuple(shape), device=pyramid.device, dtype=torch.float32)
    with _timed('msssim_loss_bwd', detail=True, nbytes=4.0 * (grad.numel() + pyr_floats + map_floats)):
        _lib.call('mrefsr_msssim_loss_bwd_f32', _p(pyramid), _p(maps), _p(mult), _p(grad_loss), b, h, w, int(bool(rgb)), levels,
                  C.c_float(loss_weight), _p(ws), C.c_int64(ws_bytes), _p(grad), _stream())
    return grad


# ------------------------------------------------------------------ LDL artifact loss of the training step (csrc/ldl_loss.hip)
LDL_TILE = (16, 32)   # pixels per block of the forward and the backward launch (rows, columns)


def _ldl_shape(name, pred, *others):
    _chk(name, pred, *others)
    if pred.dim() != 4 or pred.shape[1] != 3 or any(t.shape != pred.shape for t in others):
        raise ValueError(f'{name}: [B,3,H,W] images of one shape expected, got {[tuple(t.shape) for t in (pred, *others)]}')
    b, _, h, w = pred.shape
    blocks = _lib.load().mrefsr_ldl_loss_blocks(b, h, w)
    if blocks <= 0:
        raise ValueError(f'{name}: unsupported shape {tuple(pred.shape)} (B <= 65535, 4 <= H, W <= 2^19, H W <= 2^30)')
    return b, h, w, blocks


def ldl_loss_fwd(pred, target, ema, loss_weight=1.0, want_grad=False, want_map=False):
    """pred, target, ema [B,3,H,W] (contiguous fp32) -> (loss, saved, w): loss a 0-dim tensor = loss_weight mean |w pred - w target|
    with the LDL artifact map w of the three images; saved: None, or with want_grad what ldl_loss_bwd reads, (m r, mu, v m) each
    [B,H,W] and the per-sample scalars [B,4]; w: None, or with want_map the map [B,1,H,W] (a second launch).  Without either the
    one launch writes no map.  Fixed summation orders (the same bits from call to call), nothing read back; the inputs are only read"""
    b, h, w, blocks = _ldl_shape('ldl_loss_fwd', pred, target, ema)
    dev = pred.device
    mr, mu = (torch.empty((b, h, w), device=dev, dtype=torch.float32) for _ in range(2)) if want_grad else (None, None)
    vm = torch.empty((b, h, w), device=dev, dtype=torch.float32) if want_grad or want_map else None
    stats = torch.empty((b, 4), device=dev, dtype=torch.float32)
    loss = torch.empty((), device=dev, dtype=torch.float32)
    part, ticket = _det_scratch(dev, 16 * blocks)
    with _timed('ldl_loss_fwd', detail=True, nbytes=4.0 * (3 * pred.numel() + (3 if want_grad else 1 if want_map else 0) * b * h * w)):
        _lib.call('mrefsr_ldl_loss_fwd_f32', _p(pred), _p(target), _p(ema), b, h, w, C.c_float(loss_weight), _p(mr), _p(mu), _p(vm), _p(stats),
                  _p(part), _p(ticket), _p(loss), _stream())
    wmap = None
    if want_map:
        wmap = torch.empty((b, 1, h, w), device=dev, dtype=torch.float32)
        with _timed('ldl_loss_map', detail=True, nbytes=8.0 * b * h * w):
            _lib.call('mrefsr_ldl_loss_map_f32', _p(vm), _p(stats), b, h, w, _p(wmap), _stream())
    return loss, ((mr, mu, vm, stats) if want_grad else None), wmap


def ldl_loss_bwd(pred, target, saved, grad_loss, loss_weight=1.0):
    """d (grad_loss * loss) / d pred [B,3,H,W] of ldl_loss_fwd from what it saved; grad_loss: the upstream gradient, a one-element
    fp32 device tensor (read by the kernel, not by the host).  One launch; every element is written once"""
    b, h, w, _ = _ldl_shape('ldl_loss_bwd', pred, target)
    _chk('ldl_loss_bwd', grad_loss, *saved)
    if grad_loss.numel() != 1 or len(saved) != 4 or any(m.shape != (b, h, w) for m in saved[:3]) or saved[3].shape != (b, 4):
        raise ValueError(f'ldl_loss_bwd: one upstream value, three maps of {(b, h, w)} and the scalars {(b, 4)} expected')
    grad = torch.empty_like(pred)
    with _timed('ldl_loss_bwd', detail=True, nbytes=4.0 * (3 * pred.numel() + 3 * b * h * w)):
        _lib.call('mrefsr_ldl_loss_bwd_f32', _p(pred), _p(target), _p(saved[0]), _p(saved[1]), _p(saved[2]), _p(saved[3]), _p(grad_loss),
                  b, h, w, C.c_float(loss_weight), _p(grad), _stream())
    return grad


# ------------------------------------------------------------------ frequency-domain losses of the training step (csrc/freq_loss.hip)
FREQ_TILE = (32, 32)    # outputs per block of every pass (rows, columns): rows of X / D, columns of D (W/2 + 1 of them) / of grad
FREQ_MAX_SIDE = 1024
_freq_tables = {}       # (device index, n) -> [n,2] fp32 (cos, sin)(2 pi r / n): constants, built once, never part of a step


def freq_twiddles(device, n):
    """[n,2] fp32 on ``device``: (cos, sin)(2 pi r / n), r = 0 .. n-1, each the fp32 rounding of the float64 value.  Built on the
    host at the first request for (device, n) and kept; the kernels index it by (j k) mod n, reduced in integers"""
    key = (device.index, int(n))
    t = _freq_tables.get(key)
    if t is None:
        ang = [2.0 * math.pi * r / n for r in range(n)]
        t = _freq_tables[key] = torch.tensor([[math.cos(a), math.sin(a)] for a in ang], dtype=torch.float64).float().to(device)
    return t


def _freq_shape(name, pred, target=None):
    _chk(name, pred, target)
    if pred.dim() != 4 or (target is not None and target.shape != pred.shape):
        raise ValueError(f'{name}: [B,C,H,W] tensors of one shape expected, got {tuple(pred.shape)}'
                         + ('' if target is None else f' and {tuple(target.shape)}'))
    b, c, h, w = pred.shape
    blocks = _lib.load().mrefsr_freq_loss_blocks(b * c, h, w)
    if blocks <= 0:
        raise ValueError(f'{name}: unsupported shape {tuple(pred.shape)} (1 <= H, W <= {FREQ_MAX_SIDE}, 1 <= B C <= 65535, B C H W <= 2^30)')
    return b * c, h, w, blocks


def _align256(n):
    return (n + 255) // 256 * 256


def freq_loss_fwd(pred, target, focal=False, norm='backward', alpha=1.0, loss_weight=1.0, want_grad=False):
    """pred, target [B,C,H,W] (contiguous fp32) -> (loss, g): loss a 0-dim tensor, with D = fft2(pred - target) over the last two
    dimensions: focal=False, loss_weight mean(|Re D| + |Im D|) / 2 in the given norm ('backward' or 'ortho'); focal=True,
    loss_weight mean(w |D|^2) in the ortho norm, w = |D|^alpha over its per-plane maximum (NaN -> 0, clamped to [0, 1]; a constant).
    g: None, or with want_grad the coefficient-gradient map [B C,H,W/2+1,2] freq_loss_bwd reads.  A dense DFT on the f32 MFMA over
    the W/2 + 1 non-redundant columns; two launches (three with focal), fixed summation orders (the same bits from call to call),
    nothing read back; pred and target are only read"""
    planes, h, w, blocks = _freq_shape('freq_loss_fwd', pred, target)
    if norm not in ('backward', 'ortho'):
        raise ValueError(f"freq_loss_fwd: norm={norm!r}; 'backward' or 'ortho'")
    dev, wh = pred.device, w // 2 + 1
    tab_h, tab_w = freq_twiddles(dev, h), freq_twiddles(dev, w)
    g = torch.empty((planes, h, wh, 2), device=dev, dtype=torch.float32) if want_grad else None
    loss = torch.empty((), device=dev, dtype=torch.float32)
    # one scratch request: T | the block partials | (focal without a map: D)
    nt, npart = _align256(8 * planes * h * wh), _align256(8 * blocks)
    buf = _scratch(dev, nt + npart + (nt if focal and not want_grad else 0))
    t, part = buf[:nt], buf[nt:nt + npart]
    gbuf = g if want_grad or not focal else buf[nt + npart:]
    ticket = _zeroed_words(dev, 'ticket', 1)
    flops = 2.0 * planes * h * w * 2 * wh + 8.0 * planes * h * h * wh
    with _timed('freq_loss_fwd', detail=True, flops=flops, nbytes=4.0 * (2 * pred.numel() + (4 + (2 if want_grad else 0)) * planes * h * wh)):
        _lib.call('mrefsr_freq_loss_fwd_f32', _p(pred), _p(target), planes, h, w, int(bool(focal)), int(norm == 'ortho'),
                  C.c_float(alpha), C.c_float(loss_weight), _p(tab_h), _p(tab_w), _p(t), _p(gbuf), int(bool(want_grad)), _p(part),
                  _p(ticket), _p(loss), _stream())
    return loss, g


def freq_loss_bwd(g, grad_loss, shape, loss_weight=1.0):
    """d (grad_loss * loss) / d pred [B,C,H,W] (``shape``) of freq_loss_fwd from its map g: loss_weight grad_loss times the adjoint
    transform Re(F_H^H g F_W^H).  grad_loss: the upstream gradient, a one-element fp32 device tensor (read by the kernel, not by the
    host).  Two launches; every element is written once"""
    _chk('freq_loss_bwd', g, grad_loss)
    grad = torch.empty(tuple(shape), device=g.device, dtype=torch.float32)
    planes, h, w, _ = _freq_shape('freq_loss_bwd', grad)
    wh = w // 2 + 1
    if grad_loss.numel() != 1 or g.shape != (planes, h, wh, 2):
        raise ValueError(f'freq_loss_bwd: one upstream value and a map of {(planes, h, wh, 2)} expected, got {tuple(g.shape)}')
    tab_h, tab_w = freq_twiddles(g.device, h), freq_twiddles(g.device, w)
    u = _scratch(g.device, 8 * planes * h * wh)
    flops = 8.0 * planes * h * h * wh + 4.0 * planes * h * w * wh
    with _timed('freq_loss_bwd', detail=True, flops=flops, nbytes=4.0 * (grad.numel() + 6 * planes * h * wh)):
        _lib.call('mrefsr_freq_loss_bwd_f32', _p(g), _p(grad_loss), planes, h, w, C.c_float(loss_weight), _p(tab_h), _p(tab_w), _p(u),
                  _p(grad), _stream())
    return grad


# ------------------------------------------------------------------ contextual loss of the training step (csrc/contextual.hip)
CX_MAX_N = 4096   # MREFSR_CX_MAX_N: positions per tap (one N x N fp32 matrix per sample is materialised in scratch)


def _cx_workspace(name, b, n, c, backward):
    need = _lib.load().mrefsr_contextual_workspace_bytes(b, n, c, 1 if backward else 0)
    if need == -2:
        raise NotImplementedError(f'{name}: a tap of {n} positions and {c} channels; at most {CX_MAX_N} positions (one N x N matrix per '
                                  'sample is materialised) and 64, 128, 256 or 512 channels')
    if need < 0:
        raise ValueError(f'{name}: B={b} N={n} C={c} (1 <= B <= 65535, N >= 2)')
    return need


def _cx_weight_sp(name, weight_sp):
    if isinstance(weight_sp, bool) or not isinstance(weight_sp, (int, float)) or not (0.0 <= weight_sp < 1.0):
        raise ValueError(f'{name}: weight_sp={weight_sp!r} is not a number in [0, 1)')
    return float(weight_sp)


def contextual_fwd(x, y, band_width, weight=1.0, loss_weight=1.0, run=None, weight_sp=0.0):
    """one tap of the contextual loss: x (features of the output), y (of the target) [B,h,w,C] contiguous fp32, C of 64 ... 512, h w
    of 2 ... CX_MAX_N -> (total, saved).  run: None for the first tap of a loss, else the running sum the previous tap's call
    returned as saved['run'] (updated in place: run += tap loss * weight); total [1] = run * loss_weight.  saved: what
    contextual_bwd reads (xn, yn, rnorm, rowf = m | Z, jmin, cxmax, imax, cx [B], tap_loss [1], run).  weight_sp in [0, 1): CoBi's
    spatial term, d = (1 - weight_sp) (1 - <xn_i, yn_j>) + weight_sp |p_i - p_j|^2 / (h^2 + w^2) on the map's own h x w grid
    (0: the plain entry point; > 0: the norms and the product are taken in double, see csrc/contextual.hip).  Six launches, fixed summation orders (the same bits from call to call), nothing read back; x and y
    are only read"""
    _chk('contextual_fwd', x, y, run)
    if x.dim() != 4 or x.shape != y.shape:
        raise ValueError(f'contextual_fwd: two [B,h,w,C] maps of one shape expected, got {tuple(x.shape)} and {tuple(y.shape)}')
    if not (isinstance(band_width, (int, float)) and 0.0 < band_width < float('inf')):
        raise ValueError(f'contextual_fwd: band_width={band_width!r} is not a finite number > 0')
    weight_sp = _cx_weight_sp('contextual_fwd', weight_sp)
    b, h, w, c = x.shape
    n, dev = h * w, x.device
    need = _cx_workspace('contextual_fwd', b, n, c, False)
    f32 = dict(device=dev, dtype=torch.float32)
    s = dict(xn=torch.empty_like(x), yn=torch.empty_like(x), rnorm=torch.empty((b, n), **f32), rowf=torch.empty((2, b, n), **f32),
             jmin=torch.empty((b, n), device=dev, dtype=torch.int32), cxmax=torch.empty((b, n), **f32),
             imax=torch.empty((b, n), device=dev, dtype=torch.int32), cx=torch.empty(b, **f32), tap_loss=torch.empty(1, **f32),
             run=run if run is not None else torch.empty(1, **f32))
    total = torch.empty(1, **f32)
    ws = _scratch(dev, need)
    outs = (_p(s['xn']), _p(s['yn']), _p(s['rnorm']), _p(s['rowf']), _p(s['jmin']), _p(s['cxmax']), _p(s['imax']), _p(s['cx']),
            _p(s['tap_loss']), C.c_float(weight), C.c_float(loss_weight), 1 if run is None else 0, _p(s['run']), _p(total), _p(ws),
            C.c_int64(need), _stream())
    with _timed('contextual_fwd', 2.0 * b * n * n * c, detail=True, nbytes=4.0 * (4 * x.numel() + 3 * b * n * n)):
        if weight_sp == 0.0:
            _lib.call('mrefsr_contextual_fwd_f32', _p(x), _p(y), b, n, c, C.c_float(band_width), *outs)
        else:
            _lib.call('mrefsr_contextual_fwd_sp_f32', _p(x), _p(y), b, h, w, c, C.c_float(band_width), C.c_float(weight_sp), *outs)
    return total, s


def contextual_bwd(saved, band_width, coef, dx, gup=None, accumulate=False, want_amax=True, weight_sp=0.0):
    """dx [B,h,w,C] (+)= d (gup * coef * tap loss) / d x of contextual_fwd from its ``saved`` (the distances are recomputed); coef:
    loss_weight times the tap's weight; gup: a one-element fp32 device tensor or None (= 1); weight_sp: the forward call's.  Four
    launches, fixed orders.  -> max |dx| [1] | None"""
    names = ('xn', 'yn', 'rnorm', 'rowf', 'cxmax', 'cx')
    _chk('contextual_bwd', dx, gup, *[saved[k] for k in names])
    _chk('contextual_bwd', saved['jmin'], saved['imax'], dtype=torch.int32)
    weight_sp = _cx_weight_sp('contextual_bwd', weight_sp)
    xn = saved['xn']
    b, h, w, c = xn.shape
    n = h * w
    if tuple(dx.shape) != tuple(xn.shape) or (gup is not None and gup.numel() != 1):
        raise ValueError(f'contextual_bwd: a gradient buffer of {tuple(xn.shape)} and one upstream value expected, got {tuple(dx.shape)}')
    need = _cx_workspace('contextual_bwd', b, n, c, True)
    amax = zeros_f32(dx.device, 1) if want_amax else None
    ws = _scratch(dx.device, need)
    rest = (_p(saved['rowf']), _p(saved['jmin']), _p(saved['cxmax']), _p(saved['imax']), _p(saved['cx']), _p(gup), C.c_float(coef), _p(dx),
            1 if accumulate else 0, _p(amax), _p(ws), C.c_int64(need), _stream())
    with _timed('contextual_bwd', 4.0 * b * n * n * c, detail=True, nbytes=4.0 * (4 * xn.numel() + 3 * b * n * n)):
        if weight_sp == 0.0:
            _lib.call('mrefsr_contextual_bwd_f32', _p(xn), _p(saved['yn']), _p(saved['rnorm']), b, n, c, C.c_float(band_width), *rest)
        else:
            _lib.call('mrefsr_contextual_bwd_sp_f32', _p(xn), _p(saved['yn']), _p(saved['rnorm']), b, h, w, c, C.c_float(band_width),
                      C.c_float(weight_sp), *rest)
    return amax


def cx_patch_channels(size):
    """the channel count of size x size RGB patches as features of a contextual tap: the smallest of 64, 128, 256, 512 >= 3 size^2"""
    if isinstance(size, bool) or not isinstance(size, int) or size < 1:
        raise ValueError(f'cx_patches: size={size!r} is not an integer >= 1')
    c = _lib.load().mrefsr_cx_patch_channels(size)
    if c < 0:
        raise NotImplementedError(f'cx_patches: patches of {size} x {size} have {3 * size * size} channels; at most 512 (size <= 13)')
    return c


def _cx_patch_geometry(name, shape, size, stride):
    cpad = cx_patch_channels(size)
    if isinstance(stride, bool) or not isinstance(stride, int) or stride < 1:
        raise ValueError(f'{name}: stride={stride!r} is not an integer >= 1')
    if len(shape) != 4 or shape[1] != 3 or shape[0] < 1 or shape[2] < size or shape[3] < size:
        raise ValueError(f'{name}: a [B,3,H,W] image with H, W >= {size} expected, got {tuple(shape)}')
    return cpad, (shape[2] - size) // stride + 1, (shape[3] - size) // stride + 1


def cx_patches(img, size, stride, norm_img=False):
    """img [B,3,H,W] -> its size x size patches at ``stride`` as NHWC features [B,oh,ow,Cpad], oh = (H - size) // stride + 1: the
    channels in F.unfold's (c, dy, dx) order, zeros from 3 size^2 on (Cpad = cx_patch_channels(size)); norm_img: (img + 1) * 0.5
    first.  One launch"""
    _chk('cx_patches', img)
    cpad, oh, ow = _cx_patch_geometry('cx_patches', img.shape, size, stride)
    b, _, h, w = img.shape
    out = torch.empty((b, oh, ow, cpad), device=img.device, dtype=torch.float32)
    with _timed('cx_patches', detail=True, nbytes=4.0 * (img.numel() + out.numel())):
        _lib.call('mrefsr_cx_patches_f32', _p(img), b, h, w, size, stride, 1 if norm_img else 0, _p(out), cpad, _stream())
    return out


def cx_patches_bwd(g, shape, size, stride, scale=1.0, out=None):
    """the adjoint of cx_patches: g [B,oh,ow,Cpad] -> d / d img [B,3,H,W] (``shape``) times ``scale``; per pixel the covering patch
    entries are added in ascending (patch row, patch column) order (a gather: no atomics), a pixel no patch covers gets 0.  out:
    a gradient image to add into (None: a new one is written).  One launch"""
    _chk('cx_patches_bwd', g, out)
    cpad, oh, ow = _cx_patch_geometry('cx_patches_bwd', tuple(shape), size, stride)
    b, _, h, w = shape
    if tuple(g.shape) != (b, oh, ow, cpad) or (out is not None and tuple(out.shape) != tuple(shape)):
        raise ValueError(f'cx_patches_bwd: a gradient of {(b, oh, ow, cpad)} and an image of {tuple(shape)} expected, got {tuple(g.shape)}')
    acc = out is not None
    if out is None:
        out = torch.empty(tuple(shape), device=g.device, dtype=torch.float32)
    with _timed('cx_patches_bwd', detail=True, nbytes=4.0 * (g.numel() + out.numel())):
        _lib.call('mrefsr_cx_patches_bwd_f32', _p(g), b, h, w, size, stride, cpad, C.c_float(scale), _p(out), 1 if acc else 0, _stream())
    return out


def _cx_stride(name, f, s):
    if isinstance(s, bool) or not isinstance(s, int) or s < 1:
        raise ValueError(f'{name}: stride={s!r} is not an integer >= 1')
    if f.dim() != 4 or f.shape[3] % 4 or f.numel() == 0:
        raise ValueError(f'{name}: a [B,h,w,C] map with C a multiple of 4 expected, got {tuple(f.shape)}')


def cx_subsample(f, s):
    """f [B,h,w,C] -> its positions (r s, c s): [B,ceil(h / s),ceil(w / s),C].  One launch"""
    _chk('cx_subsample', f)
    _cx_stride('cx_subsample', f, s)
    b, h, w, c = f.shape
    out = torch.empty((b, (h + s - 1) // s, (w + s - 1) // s, c), device=f.device, dtype=torch.float32)
    with _timed('cx_subsample', detail=True, nbytes=8.0 * out.numel()):
        _lib.call('mrefsr_cx_subsample_f32', _p(f), b, h, w, c, s, _p(out), _stream())
    return out


def cx_subsample_bwd(gs, g, s, accumulate=False, want_amax=True):
    """the adjoint of cx_subsample into the tap's gradient buffer g [B,h,w,C]: written (gs at the sampled positions, zeros elsewhere)
    or, with accumulate, gs added at the sampled positions only.  -> max |g| [1] over the whole buffer | None.  One launch"""
    _chk('cx_subsample_bwd', gs, g)
    _cx_stride('cx_subsample_bwd', g, s)
    b, h, w, c = g.shape
    if tuple(gs.shape) != (b, (h + s - 1) // s, (w + s - 1) // s, c):
        raise ValueError(f'cx_subsample_bwd: a gradient of {(b, (h + s - 1) // s, (w + s - 1) // s, c)} expected, got {tuple(gs.shape)}')
    amax = zeros_f32(g.device, 1) if want_amax else None
    with _timed('cx_subsample_bwd', detail=True, nbytes=4.0 * (gs.numel() + 2 * g.numel())):
        _lib.call('mrefsr_cx_subsample_bwd_f32', _p(gs), b, h, w, c, s, _p(g), 1 if accumulate else 0, _p(amax), _stream())
    return amax


# ------------------------------------------------------------------ second-order degradation (csrc/degrade.hip; degradation.py)
DEGRADE_MODES = {'area': 0, 'bilinear': 1, 'bicubic': 2}


def _degrade_image(name, img, channels=None):
    _chk(name, img)
    if img.dim() != 4 or (channels is not None and img.shape[1] != channels) or img.numel() == 0:
        raise ValueError(f'{name}: a [B,{channels or "C"},H,W] image expected, got {tuple(img.shape)}')
    return tuple(img.shape)


def degrade_filter2d(img, kernel):
    """filter2D (basicsr/utils/img_process_util.py:7-31): img [B,C,H,W], kernel [B,k,k] or [1,k,k] (one for the batch), k odd,
    3 ... 21, H, W > k // 2 -> the k x k correlation of the reflect-padded image.  One launch"""
    b, c, h, w = _degrade_image('degrade_filter2d', img)
    _chk('degrade_filter2d', kernel)
    k = kernel.shape[-1]
    if kernel.dim() != 3 or kernel.shape[1] != k or kernel.shape[0] not in (1, b):
        raise ValueError(f'degrade_filter2d: kernels [{b},k,k] or [1,k,k] expected, got {tuple(kernel.shape)}')
    out = torch.empty_like(img)
    with _timed('degrade_filter2d', detail=True, flops=2.0 * img.numel() * k * k, nbytes=8.0 * img.numel()):
        _lib.call('mrefsr_degrade_filter2d_f32', _p(img), _p(kernel), b, c, h, w, k, int(kernel.shape[0] == 1 and b > 1), _p(out), _stream())
    return out


def degrade_usm(img, radius=51, weight=0.5, threshold=10.0):
    """USMSharp.forward (img_process_util.py:63-83; an even radius is raised by one, as there): the Gaussian as a row and a column
    pass in LDS.  img [B,C,H,W], H, W > radius // 2.  Two launches"""
    from .degradation import gaussian_kernel1d
    b, c, h, w = _degrade_image('degrade_usm', img)
    k = int(radius) + (1 if int(radius) % 2 == 0 else 0)
    if k < 3 or k > 51:
        raise ValueError(f'degrade_usm: radius {radius} outside 3 ... 51')
    taps = (C.c_float * k)(*gaussian_kernel1d(k).tolist())
    residual, out = torch.empty_like(img), torch.empty_like(img)
    with _timed('degrade_usm', detail=True, flops=8.0 * img.numel() * k, nbytes=20.0 * img.numel()):
        _lib.call('mrefsr_degrade_usm_f32', _p(img), taps, b, c, h, w, k, C.c_float(weight), C.c_float(threshold), _p(residual), _p(out),
                  _stream())
    return out


def degrade_resize_geometry(in_hw, size=None, scale_factor=None):
    """((out_h, out_w), (scale_h, scale_w)) of F.interpolate(size=... | scale_factor=..., align_corners=False): the output size and
    the output -> input coordinate scales torch uses -- 1 / scale_factor when called with scale_factor (the output size is
    floor(in * scale_factor)), in / out when called with size"""
    if (size is None) == (scale_factor is None):
        raise ValueError('degrade_resize: exactly one of size and scale_factor')
    if size is not None:
        oh, ow = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
        if oh < 1 or ow < 1:
            raise ValueError(f'degrade_resize: output size {(oh, ow)}')
        return (oh, ow), (in_hw[0] / oh, in_hw[1] / ow)
    sf = (float(scale_factor),) * 2 if isinstance(scale_factor, (int, float)) else (float(scale_factor[0]), float(scale_factor[1]))
    if not all(s > 0 and math.isfinite(s) for s in sf):
        raise ValueError(f'degrade_resize: scale_factor {scale_factor}')
    oh, ow = int(math.floor(in_hw[0] * sf[0])), int(math.floor(in_hw[1] * sf[1]))
    if oh < 1 or ow < 1:
        raise ValueError(f'degrade_resize: scale_factor {scale_factor} leaves no pixel of {tuple(in_hw)}')
    return (oh, ow), (1.0 / sf[0], 1.0 / sf[1])


def degrade_resize(img, size=None, scale_factor=None, mode='bicubic'):
    """F.interpolate(img, size=... | scale_factor=..., mode='area' | 'bilinear' | 'bicubic') with align_corners=False and no
    antialiasing (cubic A = -0.75; area = adaptive_avg_pool2d).  One launch"""
    b, c, h, w = _degrade_image('degrade_resize', img)
    if mode not in DEGRADE_MODES:
        raise ValueError(f'degrade_resize: mode {mode!r} not in {sorted(DEGRADE_MODES)}')
    (oh, ow), (sh, sw) = degrade_resize_geometry((h, w), size, scale_factor)
    out = torch.empty((b, c, oh, ow), device=img.device, dtype=torch.float32)
    with _timed('degrade_resize', detail=True, nbytes=4.0 * (img.numel() + out.numel())):
        _lib.call('mrefsr_degrade_resize_f32', _p(img), b, c, h, w, oh, ow, DEGRADE_MODES[mode], C.c_float(sh), C.c_float(sw), _p(out),
                  _stream())
    return out


def degrade_levels(img):
    """img [B,3,H,W] -> vals [B,2] fp32 on the device: 2^ceil(log2(n)) for n = the distinct values of clamp(round(img 255), 0, 255)
    over the three channels, and over the gray image 0.2989 R + 0.587 G + 0.114 B (degradations.py:630-648 without its host loop)"""
    b, _, h, w = _degrade_image('degrade_levels', img, 3)
    sets = _zeroed_words(img.device, 'levels', _lib.load().mrefsr_degrade_levels_workspace_words(b))
    vals = torch.empty((b, 2), device=img.device, dtype=torch.float32)
    with _timed('degrade_levels', detail=True, nbytes=4.0 * img.numel()):
        _lib.call('mrefsr_degrade_levels_f32', _p(img), b, h, w, _p(sets), _p(vals), _stream())
    return vals


def degrade_noise(img, noise, noise_gray, param, gray, vals=None, poisson=False):
    """The noise models of degradations.py on drawn tensors: img, noise [B,3,H,W], noise_gray [B,1,H,W], param (sigma_b, or scale_b
    with poisson), gray (flags 0 / 1) [B], vals [B,2] from degrade_levels (Poisson only).  One launch; see degradation.noise_torch"""
    b, _, h, w = _degrade_image('degrade_noise', img, 3)
    _chk('degrade_noise', noise, noise_gray, param, gray, vals)
    if noise.shape != img.shape or tuple(noise_gray.shape) != (b, 1, h, w) or tuple(param.shape) != (b,) or tuple(gray.shape) != (b,):
        raise ValueError(f'degrade_noise: noise {tuple(img.shape)}, noise_gray {(b, 1, h, w)}, param and gray {(b,)} expected')
    if poisson and (vals is None or tuple(vals.shape) != (b, 2)):
        raise ValueError(f'degrade_noise: the Poisson model needs vals {(b, 2)} (degrade_levels)')
    out = torch.empty_like(img)
    with _timed('degrade_noise', detail=True, nbytes=4.0 * (3 * img.numel() + noise_gray.numel())):
        _lib.call('mrefsr_degrade_noise_f32', _p(img), _p(noise), _p(noise_gray), _p(param), _p(gray), _p(vals if poisson else None), b, h, w,
                  1 if poisson else 0, _p(out), _stream())
    return out


def degrade_jpeg(img, quality):
    """DiffJPEG(differentiable=False) (basicsr/utils/diffjpeg.py:449-491): img [B,3,H,W] in [0, 1], quality [B] on the device
    (0 < q <= 100; not modified, where the reference overwrites it with the factors).  One launch"""
    b, _, h, w = _degrade_image('degrade_jpeg', img, 3)
    _chk('degrade_jpeg', quality)
    if tuple(quality.shape) != (b,):
        raise ValueError(f'degrade_jpeg: quality {(b,)} expected, got {tuple(quality.shape)}')
    out = torch.empty_like(img)
    with _timed('degrade_jpeg', detail=True, nbytes=8.0 * img.numel()):
        _lib.call('mrefsr_degrade_jpeg_f32', _p(img), _p(quality), b, h, w, _p(out), _stream())
    return out


def texture_swap_nhwc(feat, sel, pidx, k, s):
    """feat [K*B,s*h,s*w,C] (the references' k-major NHWC maps, read in place), sel / pidx int32 [B,h-2,w-2] from texture_select ->
    [B,s*h,s*w,C]: the matched 3s x 3s reference patches pasted at (s*y, s*x), overlaps averaged (ascending (y, x), fp32)"""
    _chk('texture_swap_nhwc', feat)
    _chk('texture_swap_nhwc', sel, pidx, dtype=torch.int32)
    if sel.dim() != 3 or sel.shape != pidx.shape or feat.dim() != 4:
        raise ValueError('texture_swap_nhwc: feat [K*B,sh,sw,C], sel / pidx [B,h-2,w-2] expected')
    b, gh, gw = sel.shape
    kb, sh, sw, c = feat.shape
    if kb != k * b or sh != s * (gh + 2) or sw != s * (gw + 2) or c % 4 or gh < 1 or gw < 1:
        raise ValueError(f'texture_swap_nhwc: feat {tuple(feat.shape)} does not fit K={k}, scale {s} and the match grid {(b, gh, gw)} '
                         '(C a multiple of 4)')
    out = torch.empty((b, sh, sw, c), device=feat.device, dtype=torch.float32)
    with _timed('texture_swap_nhwc', detail=True, nbytes=4.0 * out.numel() * (1 + 9)):
        _lib.call('mrefsr_texture_swap_nhwc_f32', _p(feat), _p(sel), _p(pidx), _p(out), k, b, gh + 2, gw + 2, s, c, _stream())
    return out


def texture_coeff(weights, scales=(1, 2, 4)):
    """weights [B,1,gh,gw] -> {s: [B,s*(gh+2),s*(gw+2)]} = sigmoid(-20 * bicubic_s(replicate_pad(weights, 1)) + 0.65)
    (align_corners=True, torch's upsample_bicubic2d), all scales in one launch"""
    _chk('texture_coeff', weights)
    if weights.dim() != 4 or weights.shape[1] != 1 or weights.shape[2] < 1 or weights.shape[3] < 1 or not set(scales) <= {1, 2, 4}:
        raise ValueError(f'texture_coeff: weights [B,1,gh,gw] and scales out of (1, 2, 4) expected, got {tuple(weights.shape)} / {scales}')
    b, _, gh, gw = weights.shape
    h, w = gh + 2, gw + 2
    outs = {s: torch.empty((b, s * h, s * w), device=weights.device, dtype=torch.float32) for s in scales}
    with _timed('texture_coeff', detail=True, nbytes=4.0 * sum(o.numel() for o in outs.values())):
        _lib.call('mrefsr_texture_coeff_f32', _p(weights), _p(outs.get(1)), _p(outs.get(2)), _p(outs.get(4)), b, h, w, _stream())
    return outs


def texture_scale_nhwc(f, coeff):
    """f [N,H,W,C] * coeff [N,H,W] (broadcast over the channels) -> [N,H,W,C]"""
    _chk('texture_scale_nhwc', f, coeff)
    if f.dim() != 4 or tuple(coeff.shape) != tuple(f.shape[:3]) or f.shape[3] % 4:
        raise ValueError(f'texture_scale_nhwc: f [N,H,W,C] (C a multiple of 4) and coeff [N,H,W] expected, got {tuple(f.shape)} / '
                         f'{tuple(coeff.shape)}')
    out = torch.empty_like(f)
    with _timed('texture_scale_nhwc', detail=True, nbytes=8.0 * f.numel()):
        _lib.call('mrefsr_texture_scale_nhwc_f32', _p(f), _p(coeff), _p(out), C.c_int64(coeff.numel()), f.shape[3], _stream())
    return out


def gram_raw_nhwc(f):
    """f [N,H,W,C] (C a multiple of 64) -> [N,C,C] = F^T F per image, not normalised: gram_nhwc's kernels with scale 1"""
    return _gram('gram_raw_nhwc', f, 1.0)


def texture_crit(gxs, gms, divs, loss_weight):
    """Gram matrices gxs[l], gms[l] [N,C_l,C_l] of up to three layers -> (norms [L] = ||gx - gm||_F over the whole tensor,
    terms [L] = norms / 4 / divs[l], total [1] = (sum(terms) / 3) * loss_weight): fixed summation order, nothing read back"""
    if not 1 <= len(gxs) <= 3 or len(gms) != len(gxs) or len(divs) != len(gxs):
        raise ValueError('texture_crit: one to three layers, as many gms and divs as gxs')
    layers = (_lib.TextureLayer * len(gxs))()
    for l, (gx, gm) in enumerate(zip(gxs, gms)):
        _chk('texture_crit', gx, gm)
        if gx.shape != gm.shape:
            raise ValueError(f'texture_crit: layer {l}: gx {tuple(gx.shape)} / gm {tuple(gm.shape)} differ')
        layers[l] = _lib.TextureLayer(gx.data_ptr(), gm.data_ptr(), gx.numel(), float(divs[l]))
    dev = gxs[0].device
    norms = torch.empty(len(gxs), device=dev, dtype=torch.float32)
    terms = torch.empty(len(gxs), device=dev, dtype=torch.float32)
    total = torch.empty(1, device=dev, dtype=torch.float32)
    part = torch.empty(3 * 64, device=dev, dtype=torch.float64)   # MREFSR_TEXTURE_MAX_LAYERS * MREFSR_TEXTURE_CRIT_BLOCKS
    with _timed('texture_crit', detail=True, nbytes=8.0 * sum(g.numel() for g in gxs)):
        _lib.call('mrefsr_texture_crit_f32', layers, len(gxs), C.c_float(loss_weight), _p(part), _p(norms), _p(terms), _p(total), _stream())
    return norms, terms, total


def texture_gram_bwd_nhwc(fc, gx, gm, coeff, norm, df, scale, gup=None, accumulate=False, want_amax=True):
    """df [N,H,W,C] (+)= d total / d f of one layer of texture_crit: coeff * (2 fc (gx - gm)) * ((gup * scale) / norm), exactly 0 where
    norm == 0.  fc = texture_scale_nhwc(f, coeff), gx = gram_raw_nhwc(fc), norm [1] the layer's entry of texture_crit's norms,
    scale = loss_weight / 3 / 4 / div, gup a device scalar or None (= 1).  -> max |df| [1] | None"""
    _chk('texture_gram_bwd_nhwc', fc, gx, gm, coeff, norm, df, gup)
    n, h, w, c = _gram_bwd_shapes('texture_gram_bwd_nhwc', fc, gx, gm, df)
    if tuple(coeff.shape) != (n, h, w) or norm.numel() != 1 or (gup is not None and gup.numel() != 1):
        raise ValueError('texture_gram_bwd_nhwc: inconsistent shapes')
    amax = zeros_f32(fc.device, 1) if want_amax else None
    with _timed('texture_gram_bwd_nhwc', 2.0 * n * h * w * c * c, detail=True, nbytes=4.0 * (2 + accumulate) * fc.numel()):
        _lib.call('mrefsr_texture_gram_bwd_nhwc_f32', _p(fc), _p(gx), _p(gm), _p(coeff), _p(norm), _p(gup), _p(df), n, h * w, c,
                  C.c_float(scale), 1 if accumulate else 0, _p(amax), _stream())
    return amax


def image_to_nhwc4_bwd(g4, range_norm=False, std=None):
    """gradient of image_to_nhwc4(img, mean, std, range_norm): g4 [N,H,W,ld>=3] (pixel-contiguous) -> [N,3,H,W]"""
    n, h, w, _ = g4.shape
    ld = _nhwc_ld('g4', g4)
    _chk('image_to_nhwc4_bwd', std)
    out = torch.empty((n, 3, h, w), device=g4.device, dtype=torch.float32)
    _lib.call('mrefsr_image_to_nhwc4_bwd_f32', _p(g4), ld, _p(out), C.c_int64(n), C.c_int64(h * w), 1 if range_norm else 0, _p(std), _stream())
    return out


# ------------------------------------------------------------------ ImageDiscriminator (csrc/disc.hip)
def disc_pack_image(img):
    """img [B,3,H,W] -> [B,H,W,4] (channel 3 = 0)"""
    _chk('disc_pack_image', img)
    b, c, h, w = img.shape
    if c != 3:
        raise NotImplementedError(f'disc_pack_image: {c} channels (the discriminator takes RGB images)')
    out = torch.empty((b, h, w, 4), device=img.device, dtype=torch.float32)
    _lib.call('mrefsr_disc_pack_image_f32', _p(img), _p(out), b, h, w, _stream())
    return out


def disc_unpack_image(g4):
    """gradient of disc_pack_image: [B,H,W,4] -> [B,3,H,W]"""
    _chk('disc_unpack_image', g4)
    b, h, w, c = g4.shape
    if c != 4:
        raise ValueError('disc_unpack_image: expected 4 channels')
    out = torch.empty((b, 3, h, w), device=g4.device, dtype=torch.float32)
    _lib.call('mrefsr_disc_unpack_image_f32', _p(g4), _p(out), b, h, w, _stream())
    return out


# ------------------------------------------------------------------ discriminator augmentation (csrc/disc_augment.hip)
def _disc_augment(name, entry, x, params, *flags):
    """params: an archs.d_augment.AugmentParams on x's device -- fpar [B,4] fp32 {db, s, c, -}, ipar [B,8] int32 {flip, ty, tx, y0,
    y1, x0, x1, -}, and the host's knowledge ``contrast`` (False: c = 1 in every sample, the per-sample sum launch is skipped)"""
    _chk(name, x, params.fpar)
    _chk(name, params.ipar, dtype=torch.int32)
    if x.dim() != 4 or x.shape[1] != 3 or x.numel() == 0:
        raise NotImplementedError(f'{name}: a non-empty [B,3,H,W] image batch expected, got {tuple(x.shape)}')
    b, _, h, w = x.shape
    if tuple(params.fpar.shape) != (b, 4) or tuple(params.ipar.shape) != (b, 8):
        raise ValueError(f'{name}: parameter tables {tuple(params.fpar.shape)} / {tuple(params.ipar.shape)} for a batch of {b} '
                         f'([{b},4] fp32 and [{b},8] int32 expected)')
    out = torch.empty_like(x)
    ws = ticket = None
    need = 0
    if params.contrast:
        need = _lib.load().mrefsr_disc_augment_workspace_bytes(b, h, w)
        if need <= 0:
            raise ValueError(f'{name}: unsupported shape {tuple(x.shape)}')
        ws, ticket = _det_scratch(x.device, need)
    _lib.call(entry, _p(x), _p(params.fpar), _p(params.ipar), b, h, w, *flags, 1 if params.contrast else 0, _p(out), _p(ws),
              C.c_int64(need), _p(ticket), _stream())
    return out


def disc_augment(x, params, bias=True):
    """x [B,3,H,W] -> T(x) of train.d_augment (archs/d_augment.py: d_augment_torch states the formulas): brightness, saturation,
    contrast, flip, integer translation and cutout with per-sample parameters; bias=False: its linear part (db taken as 0).  One
    launch, two when a sample may have contrast; fixed summation order, no atomics"""
    return _disc_augment('disc_augment', 'mrefsr_disc_augment_f32', x, params, 1 if bias else 0)


def disc_augment_adj(g, params):
    """the adjoint of disc_augment's linear part: g [B,3,H,W] (the gradient of T(x)) -> the gradient of x; launches as disc_augment"""
    return _disc_augment('disc_augment_adj', 'mrefsr_disc_augment_adj_f32', g, params)


def disc_conv_pack_weight(w, cin, dgrad):
    """w [Cout,CinR,3,3] -> [9,cin,Cout] (dgrad False) or [9,Cout,cin] (dgrad True), channels CinR..cin-1 zero"""
    _chk('disc_conv_pack_weight', w)
    cout, cinr = w.shape[:2]
    if tuple(w.shape[2:]) != (3, 3) or cinr > cin:
        raise ValueError(f'disc_conv_pack_weight: weight {tuple(w.shape)} for {cin} input channels')
    out = torch.empty((9, cout, cin) if dgrad else (9, cin, cout), device=w.device, dtype=torch.float32)
    _lib.call('mrefsr_disc_conv_pack_weight_f32', _p(w), _p(out), cout, cinr, cin, 1 if dgrad else 0, _stream())
    return out


def _disc_out(n, s):
    return (n + 1) // 2 if s == 2 else n


def disc_conv3x3(x, wpk, bias, stride):
    """x [N,H,W,Cin] -> [N,ceil(H/s),ceil(W/s),Cout]: 3x3, pad 1, + bias (wpk from disc_conv_pack_weight(dgrad=False))"""
    _chk('disc_conv3x3', x, wpk, bias)
    n, h, w, cin = x.shape
    cout = wpk.shape[2]
    if tuple(wpk.shape) != (9, cin, cout):
        raise ValueError('disc_conv3x3: packed weight does not match the input channels')
    y = torch.empty((n, _disc_out(h, stride), _disc_out(w, stride), cout), device=x.device, dtype=torch.float32)
    with _timed('disc_conv3x3', 2.0 * y.numel() * 9 * cin, detail=True):
        _lib.call('mrefsr_disc_conv3x3_f32', _p(x), _p(wpk), _p(bias), _p(y), n, h, w, cin, cout, stride, _stream())
    return y


def disc_conv3x3_dgrad(dy, wpk_d, in_shape, stride):
    """input gradient: dy [N,Ho,Wo,Cout] -> dx [N,H,W,Cin] (in_shape = x's shape; wpk_d from disc_conv_pack_weight(dgrad=True))"""
    _chk('disc_conv3x3_dgrad', dy, wpk_d)
    n, h, w, cin = in_shape
    cout = dy.shape[3]
    if tuple(dy.shape) != (n, _disc_out(h, stride), _disc_out(w, stride), cout) or tuple(wpk_d.shape) != (9, cout, cin):
        raise ValueError('disc_conv3x3_dgrad: inconsistent shapes')
    dx = torch.empty((n, h, w, cin), device=dy.device, dtype=torch.float32)
    with _timed('disc_conv3x3_dgrad', 2.0 * dy.numel() * 9 * cin, detail=True):
        _lib.call('mrefsr_disc_conv3x3_dgrad_f32', _p(dy), _p(wpk_d), _p(dx), n, h, w, cin, cout, stride, _stream())
    return dx


def disc_conv3x3_wgrad(x, dy, cin_real, stride):
    """weight gradient [Cout,cin_real,3,3] = sum over pixels of x (x) dy"""
    _chk('disc_conv3x3_wgrad', x, dy)
    n, h, w, cin = x.shape
    cout = dy.shape[3]
    if tuple(dy.shape) != (n, _disc_out(h, stride), _disc_out(w, stride), cout):
        raise ValueError('disc_conv3x3_wgrad: inconsistent shapes')
    lib = _lib.load()
    need = lib.mrefsr_disc_conv3x3_wgrad_workspace_bytes(n, h, w, cin, cout, stride)
    ws = _scratch(x.device, need)
    dw = torch.empty((cout, cin_real, 3, 3), device=x.device, dtype=torch.float32)
    with _timed('disc_conv3x3_wgrad', 2.0 * dy.numel() * 9 * cin, detail=True):
        _lib.call('mrefsr_disc_conv3x3_wgrad_f32', _p(x), _p(dy), _p(dw), n, h, w, cin, cin_real, cout, stride, _p(ws), C.c_int64(need),
                  _stream())
    return dw


def _chan_ws(t):
    p, c = t.numel() // t.shape[-1], t.shape[-1]
    need = _lib.load().mrefsr_disc_chan_workspace_bytes(p, c)
    return p, c, _scratch(t.device, need), C.c_int64(need)


def disc_bias_grad(dy):
    """[..., C] -> [C] sum over every other dimension"""
    _chk('disc_bias_grad', dy)
    p, c, ws, need = _chan_ws(dy)
    db = torch.empty(c, device=dy.device, dtype=torch.float32)
    _lib.call('mrefsr_disc_bias_grad_f32', _p(dy), _p(db), C.c_int64(p), c, _p(ws), need, _stream())
    return db


def disc_bn_lrelu(x, gamma, beta, running_mean=None, running_var=None, num_batches_tracked=None, eps=1e-5, momentum=0.1, slope=0.2):
    """BatchNorm2d (training mode) + LeakyReLU on x [N,H,W,C] -> (y, mean [C], invstd [C]); the running statistics (and
    num_batches_tracked, int64) are updated in place when given"""
    _chk('disc_bn_lrelu', x, gamma, beta, running_mean, running_var)
    if num_batches_tracked is not None:
        _chk('disc_bn_lrelu', num_batches_tracked, dtype=torch.int64)
    p, c, ws, need = _chan_ws(x)
    y = torch.empty_like(x)
    mean = torch.empty(c, device=x.device, dtype=torch.float32)
    invstd = torch.empty(c, device=x.device, dtype=torch.float32)
    with _timed('disc_bn_lrelu', detail=True):
        _lib.call('mrefsr_disc_bn_lrelu_f32', _p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(invstd), _p(running_mean), _p(running_var),
                  _p(num_batches_tracked), C.c_int64(p), c, C.c_float(eps), C.c_float(momentum), C.c_float(slope), _p(ws), need,
                  _stream())
    return y, mean, invstd


def disc_bn_lrelu_bwd(gy, y, x, mean, invstd, gamma, slope=0.2, want_gx=True, want_params=True):
    """-> (gx | None, ggamma | None, gbeta | None)"""
    _chk('disc_bn_lrelu_bwd', gy, y, x, mean, invstd, gamma)
    p, c, ws, need = _chan_ws(x)
    gx = torch.empty_like(x) if want_gx else None
    gg = torch.empty(c, device=x.device, dtype=torch.float32) if want_params else None
    gb = torch.empty(c, device=x.device, dtype=torch.float32) if want_params else None
    with _timed('disc_bn_lrelu_bwd', detail=True):
        _lib.call('mrefsr_disc_bn_lrelu_bwd_f32', _p(gy), _p(y), _p(x), _p(mean), _p(invstd), _p(gamma), _p(gx), _p(gg), _p(gb), C.c_int64(p), c,
                  C.c_float(slope), _p(ws), need, _stream())
    return gx, gg, gb


def disc_bn_lrelu_dbl(ggx, ggamma, gbeta, gy, y, x, mean, invstd, gamma, slope=0.2, want=(True, True, True)):
    """double backward: (ggx [N,H,W,C], ggamma [C] | None, gbeta [C] | None) -> (d gy, d x, d gamma), each None unless wanted"""
    _chk('disc_bn_lrelu_dbl', ggx, ggamma, gbeta, gy, y, x, mean, invstd, gamma)
    p, c, ws, need = _chan_ws(x)
    d_gy = torch.empty_like(x) if want[0] else None
    d_x = torch.empty_like(x) if want[1] else None
    d_g = torch.empty(c, device=x.device, dtype=torch.float32) if want[2] else None
    with _timed('disc_bn_lrelu_dbl', detail=True):
        _lib.call('mrefsr_disc_bn_lrelu_dbl_f32', _p(ggx), _p(ggamma), _p(gbeta), _p(gy), _p(y), _p(x), _p(mean), _p(invstd), _p(gamma), _p(d_gy),
                  _p(d_x), _p(d_g), C.c_int64(p), c, C.c_float(slope), _p(ws), need, _stream())
    return d_gy, d_x, d_g


def disc_head(f, w1, b1, w2, b2, slope=0.2):
    """f [N,H,W,C] -> (out [N], pooled [N,C], hidden [N,J]); w1 [J,C], w2 [J] (contiguous views of the 1x1 weights)"""
    _chk('disc_head', f, w1, b1, w2, b2)
    n, h, w, c = f.shape
    j = w1.shape[0]
    out = torch.empty(n, device=f.device, dtype=torch.float32)
    pooled = torch.empty((n, c), device=f.device, dtype=torch.float32)
    hidden = torch.empty((n, j), device=f.device, dtype=torch.float32)
    _lib.call('mrefsr_disc_head_fwd_f32', _p(f), _p(w1), _p(b1), _p(w2), _p(b2), _p(out), _p(pooled), _p(hidden), n, h * w, c, j, C.c_float(slope),
              _stream())
    return out, pooled, hidden


def disc_head_bwd(gs, s, pooled, hidden, w1, w2, f_shape, slope=0.2, want_params=True):
    """-> (gf [N,H,W,C], gw1 [J,C], gb1 [J], gw2 [J], gb2 [1]) (the parameter gradients None unless wanted)"""
    _chk('disc_head_bwd', gs, s, pooled, hidden, w1, w2)
    n, h, w, c = f_shape
    j = w1.shape[0]
    dev = gs.device
    gf = torch.empty((n, h, w, c), device=dev, dtype=torch.float32)
    pw = [torch.empty(sh, device=dev, dtype=torch.float32) for sh in ((j, c), (j, ), (j, ), (1, ))] if want_params else [None] * 4
    need = _lib.load().mrefsr_disc_head_workspace_bytes(n, c, j)
    _lib.call('mrefsr_disc_head_bwd_f32', _p(gs), _p(s), _p(pooled), _p(hidden), _p(w1), _p(w2), _p(gf), *[_p(t) for t in pw], n, h * w, c, j,
              C.c_float(slope), _p(_scratch(dev, need)), C.c_int64(need), _stream())
    return (gf, *pw)


def disc_head_dbl(ggf, gs, s, pooled, hidden, w1, w2, slope=0.2, want_gs=True, want_f=True, want_params=True):
    """double backward for an upstream gradient ggf [N,H,W,C] of gf alone -> (d gs [N], d f [N,H,W,C], d w1, d b1, d w2, d b2)"""
    _chk('disc_head_dbl', ggf, gs, s, pooled, hidden, w1, w2)
    n, h, w, c = ggf.shape
    j = w1.shape[0]
    dev = ggf.device
    d_gs = torch.empty(n, device=dev, dtype=torch.float32) if want_gs else None
    d_f = torch.empty_like(ggf) if want_f else None
    pw = [torch.empty(sh, device=dev, dtype=torch.float32) for sh in ((j, c), (j, ), (j, ), (1, ))] if want_params else [None] * 4
    need = _lib.load().mrefsr_disc_head_workspace_bytes(n, c, j)
    _lib.call('mrefsr_disc_head_dbl_f32', _p(ggf), _p(gs), _p(s), _p(pooled), _p(hidden), _p(w1), _p(w2), _p(d_gs), _p(d_f), *[_p(t) for t in pw], n,
              h * w, c, j, C.c_float(slope), _p(_scratch(dev, need)), C.c_int64(need), _stream())
    return (d_gs, d_f, *pw)


# ------------------------------------------------------------------ VGGStyleDiscriminator (csrc/disc_vgg.hip)
# The convolutions of disc_vgg.hip and disc_sg2.hip are one implicit GEMM (csrc/disc_conv_gemm.h) behind two families of entry
# points, and one implementation here behind the two families of wrappers.
class _ConvFamily:
    """name: the prefix of the C symbols and of the _timed names; pack: the weight packing's name; layers: ks -> (stride, pad);
    res: the forward entry point takes a residual.  (The symbols' names are put together once: the wrappers run hundreds of times
    in a discriminator step that waits for the host.)"""

    def __init__(self, name, pack, layers, res):
        self.name, self.pack, self.layers, self.res = name, pack, layers, res
        self.dgrad, self.wgrad = f'{name}_dgrad', f'{name}_wgrad'
        self.sym_pack, self.sym_fwd, self.sym_dgrad, self.sym_wgrad = (f'mrefsr_{k}_f32' for k in (pack, name, self.dgrad, self.wgrad))
        self.ws_bytes, self.wgrad_ws_bytes = f'mrefsr_{name}_workspace_bytes', f'mrefsr_{name}_wgrad_workspace_bytes'

    def out(self, h, w, ks):
        if ks not in self.layers:
            return h, w   # (the library refuses the call and says why)
        stride, pad = self.layers[ks]
        return (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1


_VCONV = _ConvFamily('disc_vconv', 'disc_vconv_pack_weight', {3: (1, 1), 4: (2, 1)}, res=False)
_SG2CONV = _ConvFamily('disc_sg2_conv', 'disc_sg2_pack_weight', {3: (2, 0), 1: (1, 0)}, res=True)


def _conv_pack_weight(fam, w, cin, dgrad):
    _chk(fam.pack, w)
    cout, cinr, ks = w.shape[0], w.shape[1], w.shape[2]
    if ks not in fam.layers or w.shape[3] != ks or cinr > cin:
        raise ValueError(f'{fam.pack}: weight {tuple(w.shape)} for {cin} input channels')
    out = torch.empty((cin, ks * ks, cout) if dgrad else (cout, ks * ks, cin), device=w.device, dtype=torch.float32)
    _lib.call(fam.sym_pack, _p(w), _p(out), cout, cinr, cin, ks, 1 if dgrad else 0, _stream())
    return out


def _conv_fwd(fam, x, wpk, bias, ks, act_slope, res=None):
    _chk(fam.name, x, wpk, bias, res)
    n, h, w, cin = x.shape
    cout = wpk.shape[0]
    if tuple(wpk.shape) != (cout, ks * ks, cin):
        raise ValueError(f'{fam.name}: packed weight does not match the input channels')
    ho, wo = fam.out(h, w, ks)
    y = torch.empty((n, ho, wo, cout), device=x.device, dtype=torch.float32)
    if res is not None and res.shape != y.shape:
        raise ValueError(f'{fam.name}: residual {tuple(res.shape)} for an output {tuple(y.shape)}')
    need = getattr(_lib.load(), fam.ws_bytes)(n, h, w, cin, cout, ks, 0)   # (may be 0: no workspace, a null pointer)
    ws, nws = (_scratch(x.device, need) if need > 0 else None), C.c_int64(max(need, 0))
    act, slope = 0 if act_slope is None else 1, C.c_float(0.0 if act_slope is None else act_slope)
    with _timed(f'{fam.name}{ks}', 2.0 * y.numel() * ks * ks * cin, detail=True):
        if fam.res:
            _lib.call(fam.sym_fwd, _p(x), _p(wpk), _p(bias), _p(res), _p(y), n, h, w, cin, cout, ks, act, slope, _p(ws), nws, _stream())
        else:
            _lib.call(fam.sym_fwd, _p(x), _p(wpk), _p(bias), _p(y), n, h, w, cin, cout, ks, act, slope, _p(ws), nws, _stream())
    return y


def _conv_dgrad(fam, dy, wpk_d, in_shape, ks, flop_div=1):
    _chk(fam.dgrad, dy, wpk_d)
    n, h, w, cin = in_shape
    cout = dy.shape[3]
    ho, wo = fam.out(h, w, ks)
    if tuple(dy.shape) != (n, ho, wo, cout) or tuple(wpk_d.shape) != (cin, ks * ks, cout):
        raise ValueError(f'{fam.dgrad}: inconsistent shapes')
    dx = torch.empty((n, h, w, cin), device=dy.device, dtype=torch.float32)
    need = getattr(_lib.load(), fam.ws_bytes)(n, h, w, cin, cout, ks, 1)
    ws = _scratch(dy.device, need) if need > 0 else None
    with _timed(f'{fam.name}{ks}_dgrad', 2.0 * dy.numel() * ks * ks * cin / flop_div, detail=True):
        _lib.call(fam.sym_dgrad, _p(dy), _p(wpk_d), _p(dx), n, h, w, cin, cout, ks, _p(ws), C.c_int64(max(need, 0)), _stream())
    return dx


def _conv_wgrad(fam, x, dy, cin_real, ks):
    _chk(fam.wgrad, x, dy)
    n, h, w, cin = x.shape
    cout = dy.shape[3]
    ho, wo = fam.out(h, w, ks)
    if tuple(dy.shape) != (n, ho, wo, cout):
        raise ValueError(f'{fam.wgrad}: inconsistent shapes')
    need = getattr(_lib.load(), fam.wgrad_ws_bytes)(n, h, w, cin, cout, ks)
    dw = torch.empty((cout, cin_real, ks, ks), device=x.device, dtype=torch.float32)
    with _timed(f'{fam.name}{ks}_wgrad', 2.0 * dy.numel() * ks * ks * cin, detail=True):
        _lib.call(fam.sym_wgrad, _p(x), _p(dy), _p(dw), n, h, w, cin, cin_real, cout, ks, _p(_scratch(x.device, need)), C.c_int64(need), _stream())
    return dw


def disc_vconv_pack_weight(w, cin, dgrad):
    """w [Cout,CinR,ks,ks] (ks 3 or 4) -> [Cout,ks*ks,cin] (dgrad False) or [cin,ks*ks,Cout] (dgrad True), channels CinR..cin-1 zero"""
    return _conv_pack_weight(_VCONV, w, cin, dgrad)


def disc_vconv(x, wpk, bias, ks, act_slope=None):
    """x [N,H,W,Cin] -> [N,Ho,Wo,Cout]: ks 3 (stride 1) or 4 (stride 2), pad 1, + bias, then LeakyReLU(act_slope) unless it is None
    (wpk from disc_vconv_pack_weight(dgrad=False))"""
    return _conv_fwd(_VCONV, x, wpk, bias, ks, act_slope)


def disc_vconv_dgrad(dy, wpk_d, in_shape, ks):
    """input gradient: dy [N,Ho,Wo,Cout] -> dx [N,H,W,Cin] (in_shape = x's shape; wpk_d from disc_vconv_pack_weight(dgrad=True))"""
    return _conv_dgrad(_VCONV, dy, wpk_d, in_shape, ks)


def disc_vconv_wgrad(x, dy, cin_real, ks):
    """weight gradient [Cout,cin_real,ks,ks] = sum over the output pixels of x (x) dy"""
    return _conv_wgrad(_VCONV, x, dy, cin_real, ks)


def disc_lrelu_mask(g, y, slope=0.2):
    """g * lrelu'(y), the mask from the sign of the LeakyReLU output y"""
    _chk('disc_lrelu_mask', g, y)
    if g.shape != y.shape:
        raise ValueError('disc_lrelu_mask: g and y differ in shape')
    out = torch.empty_like(g)
    _lib.call('mrefsr_disc_lrelu_mask_f32', _p(g), _p(y), _p(out), C.c_int64(g.numel()), C.c_float(slope), _stream())
    return out


def disc_linear_head(f, w1, b1, w2, b2, slope=0.2):
    """f [N,H,W,C] -> (out [N], hidden [N,J]): linear2(lrelu(linear1(f flattened in NCHW order))); w1 [J,C*H*W] (torch's layout),
    w2 [J] (a contiguous view of linear2.weight)"""
    _chk('disc_linear_head', f, w1, b1, w2, b2)
    n, h, w, c = f.shape
    j = w1.shape[0]
    if tuple(w1.shape) != (j, c * h * w) or tuple(w2.shape) != (j, ):
        raise RuntimeError(f'disc_linear_head: linear1 expects {w1.shape[1]} input features, the map [{n},{c},{h},{w}] gives {c * h * w}')
    out = torch.empty(n, device=f.device, dtype=torch.float32)
    hidden = torch.empty((n, j), device=f.device, dtype=torch.float32)
    _lib.call('mrefsr_disc_linear_head_fwd_f32', _p(f), _p(w1), _p(b1), _p(w2), _p(b2), _p(out), _p(hidden), n, h * w, c, j, C.c_float(slope),
              _stream())
    return out, hidden


def disc_linear_head_bwd(gs, hidden, f, w1, w2, slope=0.2, want_f=True, want_params=True):
    """-> (gf [N,H,W,C] | None, gw1 [J,K], gb1 [J], gw2 [J], gb2 [1]) (the parameter gradients None unless wanted)"""
    _chk('disc_linear_head_bwd', gs, hidden, f, w1, w2)
    n, h, w, c = f.shape
    j = w1.shape[0]
    dev = gs.device
    gf = torch.empty_like(f) if want_f else None
    pw = [torch.empty(sh, device=dev, dtype=torch.float32) for sh in ((j, c * h * w), (j, ), (j, ), (1, ))] if want_params else [None] * 4
    _lib.call('mrefsr_disc_linear_head_bwd_f32', _p(gs), _p(hidden), _p(f), _p(w1), _p(w2), _p(gf), *[_p(t) for t in pw], n, h * w, c, j,
              C.c_float(slope), _stream())
    return (gf, *pw)


def disc_linear_head_dbl(ggf, gs, hidden, w1, w2, slope=0.2, want_gs=True, want_params=True):
    """double backward for an upstream gradient ggf [N,H,W,C] of gf alone -> (d gs [N], d w1 [J,K], d w2 [J]), each None unless wanted"""
    _chk('disc_linear_head_dbl', ggf, gs, hidden, w1, w2)
    n, h, w, c = ggf.shape
    j = w1.shape[0]
    dev = ggf.device
    d_gs = torch.empty(n, device=dev, dtype=torch.float32) if want_gs else None
    d_w1 = torch.empty((j, c * h * w), device=dev, dtype=torch.float32) if want_params else None
    d_w2 = torch.empty(j, device=dev, dtype=torch.float32) if want_params else None
    need = _lib.load().mrefsr_disc_linear_head_workspace_bytes(n, j)
    _lib.call('mrefsr_disc_linear_head_dbl_f32', _p(ggf), _p(gs), _p(hidden), _p(w1), _p(w2), _p(d_gs), _p(d_w1), _p(d_w2), n, h * w, c, j,
              C.c_float(slope), _p(_scratch(dev, need)), C.c_int64(need), _stream())
    return d_gs, d_w1, d_w2


# ------------------------------------------------------------------ validation metrics (csrc/metrics.hip)
VALM_SSIM_Y, VALM_SSIM_RGB = 1, 2


def tensor2img_u8(x):
    """x [N,C,H,W] fp32 -> [N,H,W,C] uint8 with the quantisation of metrics.tensor2img"""
    _chk('tensor2img', x)
    if x.dim() != 4:
        raise ValueError(f'tensor2img: expected [N,C,H,W], got {tuple(x.shape)}')
    n, c, h, w = x.shape
    img = torch.empty((n, h, w, c), device=x.device, dtype=torch.uint8)
    _lib.call('mrefsr_tensor2img_u8', _p(x), _p(img), n, c, h, w, _stream())
    return img


def val_metrics(out, gt, crop_border, sizes=None, flags=VALM_SSIM_Y, want_img=False):
    """out [N,3,H,W], gt [N,3,Hg,Wg] fp32; sizes: None or N pairs (oh, ow), the valid region of each image ->
    (res int64 [N,8] on the device: the rows of mrefsr_val_metrics_f32, the output's uint8 image [N,H,W,3] or None)"""
    _chk('val_metrics', out, gt)
    if out.dim() != 4 or gt.dim() != 4 or out.shape[1] != 3 or gt.shape[1] != 3 or out.shape[0] != gt.shape[0]:
        raise ValueError(f'val_metrics: expected [N,3,H,W] output and GT, got {tuple(out.shape)} and {tuple(gt.shape)}')
    n, _, h, w = out.shape
    hg, wg = gt.shape[2:]
    sz = C.c_void_p(0)
    if sizes is not None:
        flat = [int(v) for s in sizes for v in tuple(s)[:2]]
        if len(flat) != 2 * n:
            raise ValueError(f'val_metrics: {len(flat) // 2} valid sizes for {n} images')
        sz_host = (C.c_int * len(flat))(*flat)     # host memory, read before the call returns
        sz = C.cast(sz_host, C.c_void_p)
    lib = _lib.load()
    need = lib.mrefsr_val_metrics_workspace_bytes(n, h, w)
    res = torch.empty((n, 8), device=out.device, dtype=torch.int64)
    img = torch.empty((n, h, w, 3), device=out.device, dtype=torch.uint8) if want_img else None
    _lib.call('mrefsr_val_metrics_f32', _p(out), _p(gt), n, h, w, hg, wg, sz, int(crop_border), int(flags), _p(img), _p(res),
              _p(_scratch(out.device, need)), C.c_int64(need), _stream())
    return res, img


# ------------------------------------------------------------------ UNetDiscriminatorSN (csrc/disc_unet.hip)
def _sn_geometry(ws):
    return (C.c_int * len(ws))(*[w.shape[0] for w in ws]), (C.c_int * len(ws))(*[w[0].numel() for w in ws])


def disc_sn_power(w_origs, us, vs, update, eps=1e-12):
    """spectral norm of the layers w_origs ([Cout,...] each, at most 8) -> (snap_u [sum Cout], snap_v [sum fan-in], sigma [L]): one
    power iteration from the buffers us, vs, written back in place, when update; else the stored u, v as they are"""
    _chk('disc_sn_power', *w_origs, *us, *vs)
    if not 1 <= len(w_origs) <= 8 or not len(w_origs) == len(us) == len(vs):
        raise ValueError('disc_sn_power: 1 to 8 layers, one u and one v each')
    for w, u, v in zip(w_origs, us, vs):
        if not (w.is_contiguous() and u.is_contiguous() and v.is_contiguous()) or u.numel() != w.shape[0] or v.numel() != w[0].numel():
            raise ValueError(f'disc_sn_power: weight {tuple(w.shape)} with u {tuple(u.shape)}, v {tuple(v.shape)}')
    rows, cols = _sn_geometry(w_origs)
    dev = w_origs[0].device
    snap_u = torch.empty(sum(rows), device=dev, dtype=torch.float32)
    snap_v = torch.empty(sum(cols), device=dev, dtype=torch.float32)
    sigma = torch.empty(len(w_origs), device=dev, dtype=torch.float32)
    need = _lib.load().mrefsr_disc_sn_workspace_bytes(rows, cols, len(w_origs))
    with _timed('disc_sn_power', 4.0 * sum(r * c for r, c in zip(rows, cols)), detail=True):
        _lib.call('mrefsr_disc_sn_power_f32', _ptrs(w_origs), _ptrs(us), _ptrs(vs), rows, cols, len(w_origs), 1 if update else 0, C.c_float(eps),
                  _p(snap_u), _p(snap_v), _p(sigma), _p(_scratch(dev, need)), C.c_int64(need), _stream())
    return snap_u, snap_v, sigma


def disc_sn_scale(w_origs, sigma):
    """[w_orig / sigma[l]] for every layer, one launch"""
    _chk('disc_sn_scale', *w_origs, sigma)
    outs = [torch.empty_like(w, memory_format=torch.contiguous_format) for w in w_origs]
    rows, cols = _sn_geometry(w_origs)
    _lib.call('mrefsr_disc_sn_scale_f32', _ptrs([_c(w) for w in w_origs]), _ptrs(outs), rows, cols, len(w_origs), _p(sigma), _stream())
    return outs


def disc_sn_bwd(gs, w_origs, snap_u, snap_v, sigma):
    """[g / sigma - (<g, w_orig> / sigma^2) u v^T] per layer (u, v, sigma from disc_sn_power)"""
    _chk('disc_sn_bwd', *gs, *w_origs, snap_u, snap_v, sigma)
    if any(g.shape != w.shape or not g.is_contiguous() or not w.is_contiguous() for g, w in zip(gs, w_origs)):
        raise ValueError('disc_sn_bwd: gradients must be contiguous and shaped like the weights')
    rows, cols = _sn_geometry(w_origs)
    dws = [torch.empty_like(w) for w in w_origs]
    need = _lib.load().mrefsr_disc_sn_bwd_workspace_bytes(rows, cols, len(w_origs))
    with _timed('disc_sn_bwd', 4.0 * sum(r * c for r, c in zip(rows, cols)), detail=True):
        _lib.call('mrefsr_disc_sn_bwd_f32', _ptrs(gs), _ptrs(w_origs), _ptrs(dws), rows, cols, len(w_origs), _p(snap_u), _p(snap_v), _p(sigma),
                  _p(_scratch(gs[0].device, need)), C.c_int64(need), _stream())
    return dws


def _aligned(name, *ts):
    for t in ts:
        if t is not None and (not t.is_contiguous() or t.data_ptr() % 16):
            raise ValueError(f'{name}: tensors must be contiguous and 16-byte aligned')


def disc_up2(y, skip=None):
    """bilinear x2 (align_corners False) of y (+ skip) [N,h,w,C] -> [N,2h,2w,C]"""
    _chk('disc_up2', y, skip)
    _aligned('disc_up2', y, skip)
    n, h, w, c = y.shape
    if skip is not None and skip.shape != y.shape:
        raise RuntimeError(f'disc_up2: the skip addend {tuple(skip.shape)} does not match {tuple(y.shape)}')
    out = torch.empty((n, 2 * h, 2 * w, c), device=y.device, dtype=torch.float32)
    with _timed('disc_up2', detail=True, nbytes=4.0 * (y.numel() * (1 if skip is None else 2) + out.numel())):
        _lib.call('mrefsr_disc_up2_f32', _p(y), _p(skip), _p(out), n, h, w, c, _stream())
    return out


def disc_up2_adj(g):
    """adjoint of disc_up2: g [N,2h,2w,C] -> [N,h,w,C]"""
    _chk('disc_up2_adj', g)
    _aligned('disc_up2_adj', g)
    n, h2, w2, c = g.shape
    if h2 % 2 or w2 % 2:
        raise ValueError(f'disc_up2_adj: {h2} x {w2} is not an upsampled size')
    out = torch.empty((n, h2 // 2, w2 // 2, c), device=g.device, dtype=torch.float32)
    with _timed('disc_up2_adj', detail=True, nbytes=4.0 * (g.numel() + out.numel())):
        _lib.call('mrefsr_disc_up2_adj_f32', _p(g), _p(out), n, h2 // 2, w2 // 2, c, _stream())
    return out


def disc_add(a, b):
    _chk('disc_add', a, b)
    if a.shape != b.shape or not a.is_contiguous() or not b.is_contiguous():
        raise RuntimeError(f'disc_add: {tuple(a.shape)} + {tuple(b.shape)}')
    out = torch.empty_like(a)
    _lib.call('mrefsr_disc_add_f32', _p(a), _p(b), _p(out), C.c_int64(a.numel()), _stream())
    return out


def disc_conv9(x, w, bias=None):
    """nn.Conv2d(C, 1, 3, 1, 1) on x [N,H,W,C] -> [N,H,W,1]; w [1,C,3,3]"""
    _chk('disc_conv9', x, w, bias)
    _aligned('disc_conv9', x)
    n, h, wd, c = x.shape
    if tuple(w.shape) != (1, c, 3, 3):
        raise ValueError(f'disc_conv9: weight {tuple(w.shape)} for {c} channels')
    y = torch.empty((n, h, wd, 1), device=x.device, dtype=torch.float32)
    with _timed('disc_conv9', 2.0 * x.numel() * 9, detail=True):
        _lib.call('mrefsr_disc_conv9_f32', _p(x), _p(_c(w)), _p(bias), _p(y), n, h, wd, c, _stream())
    return y


def disc_conv9_dgrad(gy, w):
    """input gradient: gy [N,H,W,1] -> [N,H,W,C]"""
    _chk('disc_conv9_dgrad', gy, w)
    n, h, wd, _ = gy.shape
    c = w.shape[1]
    dx = torch.empty((n, h, wd, c), device=gy.device, dtype=torch.float32)
    with _timed('disc_conv9_dgrad', 2.0 * dx.numel() * 9, detail=True):
        _lib.call('mrefsr_disc_conv9_dgrad_f32', _p(_c(gy)), _p(_c(w)), _p(dx), n, h, wd, c, _stream())
    return dx


def disc_conv9_wgrad(x, gy):
    """weight gradient [1,C,3,3] = sum over the pixels of x (x) gy"""
    _chk('disc_conv9_wgrad', x, gy)
    _aligned('disc_conv9_wgrad', x)
    n, h, wd, c = x.shape
    if tuple(gy.shape) != (n, h, wd, 1):
        raise ValueError('disc_conv9_wgrad: inconsistent shapes')
    need = _lib.load().mrefsr_disc_conv9_wgrad_workspace_bytes(n, h, wd, c)
    dw = torch.empty((1, c, 3, 3), device=x.device, dtype=torch.float32)
    with _timed('disc_conv9_wgrad', 2.0 * x.numel() * 9, detail=True):
        _lib.call('mrefsr_disc_conv9_wgrad_f32', _p(x), _p(_c(gy)), _p(dw), n, h, wd, c, _p(_scratch(x.device, need)), C.c_int64(need), _stream())
    return dw


# ------------------------------------------------------------------ StyleGAN2Discriminator (csrc/disc_sg2.hip)
def disc_sg2_fir_out(n, taps, pad, down):
    return (n + pad[0] + pad[1] - len(taps)) // down + 1


def disc_sg2_fir(x, taps, pad, down=1, adjoint_shape=None):
    """upfirdn2d(x, outer(taps, taps), down=down, pad=pad) on channels-last x [N,H,W,C] with 2 .. 4 normalised taps (a sequence of
    floats).  adjoint_shape (N, H, W, C): x is a gradient of that operation's output instead and the result its input gradient"""
    _chk('disc_sg2_fir', x)
    taps = [float(t) for t in taps]
    n, h, w, c = x.shape if adjoint_shape is None else adjoint_shape
    ho, wo = disc_sg2_fir_out(h, taps, pad, down), disc_sg2_fir_out(w, taps, pad, down)
    if adjoint_shape is not None and tuple(x.shape) != (n, ho, wo, c):
        raise ValueError('disc_sg2_fir: the gradient does not have the output shape of the FIR')
    y = torch.empty((n, ho, wo, c) if adjoint_shape is None else (n, h, w, c), device=x.device, dtype=torch.float32)
    k = (C.c_float * len(taps))(*taps)
    with _timed('disc_sg2_fir', 2.0 * y.numel() * len(taps) ** 2, detail=True):
        _lib.call('mrefsr_disc_sg2_fir_f32', _p(x), _p(y), n, h, w, c, C.cast(k, C.c_void_p), len(taps), pad[0], pad[1], down,
                  0 if adjoint_shape is None else 1, _stream())
    return y


def disc_sg2_pack_weight(w, cin, dgrad):
    """w [Cout,CinR,ks,ks] (ks 1 or 3) -> [Cout,ks*ks,cin] (dgrad False) or [cin,ks*ks,Cout] (dgrad True), channels CinR..cin-1 zero"""
    return _conv_pack_weight(_SG2CONV, w, cin, dgrad)


def disc_sg2_conv(x, wpk, bias, ks, act_slope=None, res=None):
    """x [N,H,W,Cin] -> [N,Ho,Wo,Cout]: pad 0, ks 3 (stride 2) or 1 (stride 1); lrelu(conv + bias, act_slope) (no activation when
    act_slope is None) + res (wpk from disc_sg2_pack_weight(dgrad=False))"""
    return _conv_fwd(_SG2CONV, x, wpk, bias, ks, act_slope, res)


def disc_sg2_conv_dgrad(dy, wpk_d, in_shape, ks):
    """input gradient: dy [N,Ho,Wo,Cout] -> dx [N,H,W,Cin] (in_shape = x's shape; wpk_d from disc_sg2_pack_weight(dgrad=True))"""
    return _conv_dgrad(_SG2CONV, dy, wpk_d, in_shape, ks, flop_div=4 if ks == 3 else 1)


def disc_sg2_conv_wgrad(x, dy, cin_real, ks):
    """weight gradient [Cout,cin_real,ks,ks] = sum over the output pixels of x (x) dy"""
    return _conv_wgrad(_SG2CONV, x, dy, cin_real, ks)
