"""HipAdam: torch.optim.Adam whose step() is one launch of this project's kernel (csrc/optim.hip, mrefsr_adam_multi_f32).

Everything but step() is torch's: the state layout (``step``, ``exp_avg``, ``exp_avg_sq`` per parameter), state_dict() /
load_state_dict(), param_groups, the schedulers that edit ``group['lr']``.  A training state saved by one of the two loads into
the other (MultiRefRestorationModel.resume_training), so a run can switch ``train.hip_adam`` at a resume.

``ema_params`` (optional): {parameter: its exponential-moving-average tensor}; the step then also writes
ema = ema_decay * ema + (1 - ema_decay) * p for each of them in the same pass over the parameters -- for parameters that took no
step as well (no gradient, or in no group: the reference's model_ema updates every parameter, base_model.py:75-82).
"""
import torch

from . import hip


class HipAdam(torch.optim.Adam):

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, ema_params=None, ema_decay=0.0, **kw):
        for k in ('amsgrad', 'maximize', 'capturable', 'differentiable', 'fused', 'decoupled_weight_decay'):
            if kw.get(k):
                raise NotImplementedError(f'HipAdam: {k} is not implemented (plain Adam with L2 weight decay)')
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)
        self.ema_params, self.ema_decay = ema_params, ema_decay

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
        jobs, rows, row_of, slots, written, n_ema = [], [], {}, [], [], 0   # jobs: (p, grad, exp_avg, exp_avg_sq, ema, row of its group)
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
                k = (lr, b1, b2, eps, wd, c[1])   # (a parameter that sat out some steps has a count, hence a row, of its own)
                r = row_of.get(k)
                if r is None:
                    r = row_of[k] = len(rows)
                    rows.append(k)
                jobs.append((p, g if g.is_contiguous() else g.contiguous(), st['exp_avg'], st['exp_avg_sq'], e, r))
                written.append(p)
        if len(ema) > n_ema:   # parameters of no group (frozen ones)
            grouped = {p for group in self.param_groups for p in group['params']}
            for p, e in ema.items():
                if p not in grouped:
                    jobs.append((p, None, None, None, e, -1))
                    written.append(e)
        if not jobs:
            return loss
        self._table = hip.optim_table(*(list(col) for col in zip(*jobs)), cached=getattr(self, '_table', None))
        if rows:
            if getattr(self, '_slots', None) != slots:
                self._slots, self._slot_index = slots, torch.tensor(slots, dtype=torch.int64)
            self._steps.index_add_(0, self._slot_index, torch.ones(len(slots)))   # every state['step'] of this update, one call
            hip.adam_multi(self._table, rows, written, float(getattr(self, 'ema_decay', 0.0) or 0.0))
        else:
            hip.ema_multi(self._table, float(self.ema_decay), written)
        return loss
