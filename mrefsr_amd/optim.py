"""HipAdam: torch.optim.Adam whose step() is one launch of this project's kernel (csrc/optim.hip, mrefsr_adam_multi_f32).

Everything but step() is torch's: the state layout (``step``, ``exp_avg``, ``exp_avg_sq`` per parameter), state_dict() /
load_state_dict(), param_groups, the schedulers that edit ``group['lr']``.  A training state saved by one of the two loads into
the other (MultiRefRestorationModel.resume_training), so a run can switch ``train.hip_adam`` at a resume.

``ema_params`` (optional): {parameter: its exponential-moving-average tensor}; the step then also writes
ema = ema_decay * ema + (1 - ema_decay) * p for each of them in the same pass over the parameters -- for parameters that took no
step as well (no gradient, or in no group: the reference's model_ema updates every parameter, base_model.py:75-82).

``max_grad_norm`` (> 0) / ``skip_nonfinite``: torch.nn.utils.clip_grad_norm_ over all groups in front of the update, and an update
left out on the device when that norm is not finite -- two launches more (hip.grad_norm_multi), no readback: the state of the
last step is ``clip_state`` (a hip.GradClipState, device scalars).  The host's step counters count a skipped step like any other;
the kernel takes them less ``clip_state.skipped``.  state_dict() (through a pre-hook: the method itself stays torch's) and
load_state_dict() fold that count into the counters and zero it -- one readback, at checkpoint time -- so a saved state holds
the steps really taken and loads into torch.optim.Adam.  ``skipped_folded``: the steps folded so far.
"""
import math

import torch

from . import hip


class HipAdam(torch.optim.Adam):

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, ema_params=None, ema_decay=0.0,
                 max_grad_norm=None, skip_nonfinite=False, **kw):
        for k in ('amsgrad', 'maximize', 'capturable', 'differentiable', 'fused', 'decoupled_weight_decay'):
            if kw.get(k):
                raise NotImplementedError(f'HipAdam: {k} is not implemented (plain Adam with L2 weight decay)')
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)
        self.ema_params, self.ema_decay = ema_params, ema_decay
        if max_grad_norm is not None and not (math.isfinite(max_grad_norm) and max_grad_norm > 0):
            raise ValueError(f'HipAdam: max_grad_norm {max_grad_norm} must be a finite number above 0 (None: no clipping)')
        self.max_grad_norm, self.skip_nonfinite = max_grad_norm, bool(skip_nonfinite)
        self.clip_state, self.skipped_folded = None, 0
        self.register_state_dict_pre_hook(HipAdam._fold_skipped)

    def _fold_skipped(self):
        """the device's count of skipped steps comes off the host counters of the parameters that took part (_slots: the same
        set since the last fold, step() sees to that) and is zeroed"""
        st = getattr(self, 'clip_state', None)
        if st is None:
            return
        k = int(st.skipped.item())
        if k == 0:
            return
        st.skipped.zero_()
        self.skipped_folded += k
        slots = set(self._slots or ())
        self._steps.index_add_(0, self._slot_index, torch.full((len(self._slots),), -float(k)))
        for c in self._seen.values():
            if c[0] is not None and c[2] in slots:
                c[1] -= k

    def load_state_dict(self, state_dict):
        self._fold_skipped()   # (the counters that arrive are true counts: the device's must be 0 when they are adopted)
        return super().load_state_dict(state_dict)

    def _adopt_counter(self, p, st, c):
        """state['step'] of one parameter becomes an element of the host tensor ``_steps``, keeping its value (torch's own 0-dim
        fp32 counters, incremented one by one, cost 2 ms per step for net_g's 350 parameters; a state written by torch's fused
        Adam counts on the device: one readback, once)"""
        value = float(st['step'])
        if c is None:
            c = self._seen[p] = [None, 0, len(self._seen)]
        if c[2] >= self._steps.numel():   # grow: the counters adopted so far move with their values
            grown = torch.zeros(max(64, 2 * self._steps.numel()))
            grown[:self._steps.numel()] = self._steps
            self._steps = grown
            for q, cq in self._seen.items():
                if cq[0] is not None and self.state[q].get('step') is cq[0]:
                    cq[0] = self.state[q]['step'] = grown[cq[2]]
        c[0] = st['step'] = self._steps[c[2]]
        c[0].fill_(value)
        c[1] = int(value)
        return c

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        ema = getattr(self, 'ema_params', None) or {}
        seen = getattr(self, '_seen', None)   # parameter -> [its state's step tensor, that tensor's value, its slot in _steps]
        if seen is None:
            seen = self._seen = {}
            self._steps = torch.zeros(0)
        clip = bool(getattr(self, 'max_grad_norm', None) or getattr(self, 'skip_nonfinite', False))
        jobs, slots, written, n_ema = [], [], [], 0   # jobs: (p, grad, exp_avg, exp_avg_sq, ema, (its group's values, its counter))
        for group in self.param_groups:
            if group.get('amsgrad') or group.get('maximize'):
                raise NotImplementedError('HipAdam: amsgrad / maximize are not implemented')
            lr, (b1, b2), eps, wd = group['lr'], group['betas'], group['eps'], group['weight_decay']
            for p in group['params']:
                g, e = p.grad, ema.get(p)
                if e is not None:
                    written.append(e)
                    n_ema += 1
                if g is None:   # torch skips it; its EMA is still due
                    if e is not None:
                        jobs.append((p, None, None, None, e, -1))
                    continue
                if g.is_sparse:
                    raise RuntimeError('Adam does not support sparse gradients, please consider SparseAdam instead')
                st = self.state[p]
                if not st:   # torch's lazy initialisation (Adam._init_group), the step counter on the host
                    st['step'] = torch.tensor(0.0, dtype=torch.float32)
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                c = seen.get(p)
                if c is None or c[0] is not st['step']:   # the first step, or a state that load_state_dict brought
                    c = self._adopt_counter(p, st, c)
                c[1] += 1
                slots.append(c[2])
                jobs.append((p, g if g.is_contiguous() else g.contiguous(), st['exp_avg'], st['exp_avg_sq'], e, ((lr, b1, b2, eps, wd), c)))
                written.append(p)
        if len(ema) > n_ema:   # parameters of no group (frozen ones)
            grouped = {p for group in self.param_groups for p in group['params']}
            for p, e in ema.items():
                if p not in grouped:
                    jobs.append((p, None, None, None, e, -1))
                    written.append(e)
        if not jobs:
            return loss
        if clip and slots and getattr(self, '_slots', None) not in (None, slots):
            self._fold_skipped()   # another set of parameters steps: the count so far belongs to the set before (rare; one readback)
        rows, row_of = [], {}
        for i, job in enumerate(jobs):
            if job[5] != -1:
                k = (*job[5][0], job[5][1][1])   # (a parameter that sat out some steps has a count, hence a row, of its own)
                r = row_of.get(k)
                if r is None:
                    r = row_of[k] = len(rows)
                    rows.append(k)
                jobs[i] = job[:5] + (r,)
        self._table = hip.optim_table(*(list(col) for col in zip(*jobs)), cached=getattr(self, '_table', None))
        if rows:
            if getattr(self, '_slots', None) != slots:
                self._slots, self._slot_index = slots, torch.tensor(slots, dtype=torch.int64)
            self._steps.index_add_(0, self._slot_index, torch.ones(len(slots)))   # every state['step'] of this update, one call
            ema_decay = float(getattr(self, 'ema_decay', 0.0) or 0.0)
            if clip:
                if self.clip_state is None:
                    self.clip_state = hip.GradClipState(self._table.table.device)
                hip.grad_norm_multi(self._table, self.clip_state, self.max_grad_norm or 0.0, self.skip_nonfinite)
                hip.adam_multi(self._table, rows, written, ema_decay, clip=self.clip_state, skip=self.skip_nonfinite)
            else:
                hip.adam_multi(self._table, rows, written, ema_decay)
        else:
            hip.ema_multi(self._table, float(self.ema_decay), written)
        return loss
