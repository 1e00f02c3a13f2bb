"""Adam and AdamW over the fused HIP kernels (vqw_adam_step / vqw_adam_multi, vqw_adamw_step / vqw_adamw_multi).

Adam: drop-in for the `torch.optim.Adam(params, lr, betas, weight_decay)` instances the
reference builds in trainers/base.py:165-175: same constructor arguments, same update
rule, same state_dict layout ('step', 'exp_avg', 'exp_avg_sq' per parameter).

AdamW: torch.optim.AdamW's constructor arguments, update rule (decoupled decay) and state_dict layout, plus `max_grad_norm`:
torch.nn.utils.clip_grad_norm_ over the parameters of ALL groups, computed on the device (vqw_grad_norm_multi) and applied inside
the update - no host read, and p.grad keeps its unclipped values.  The GPT code prior's optimiser (trainers/prior.py).

Both share one base: the state's creation, the stock-optimiser state loader, the 40-byte chunk rows and the pinned ring the
pointer table goes up through.
"""
import os

import numpy as np
import torch

from . import ops as _ops


# One multi-tensor launch per parameter group (VQW_ADAM_MULTI, default on since round 3) needs a pointer table uploaded every
# step (gradient tensors are new every step; a small ring of pinned buffers).  Measured on the 95 ms step of round 3:
# 95.36 / 95.13 ms per-tensor (147 launches of ~3 us at the very end of the step, where nothing overlaps them) against
# 95.04 / 94.88 ms multi-tensor.  VQW_ADAM_MULTI=0 restores the per-tensor launches; a group whose tensors do not share a
# step count or a layout falls back to them by itself.
MULTI_TENSOR = os.environ.get("VQW_ADAM_MULTI", "1") != "0"
# elements per workgroup of the multi-tensor launch: ~950 workgroups for the R-cfg model; 8 192 ... 65 536 measure the same
# step time - the optimiser's launches overlap the next step's first kernels
CHUNK = 1 << 14


def _same_layout(a, b):
    """Same element order in memory: equal strides on every dimension of size > 1 (a size-1 dimension's stride is
    arbitrary: a (16, 1, 3, 3) weight is 'channels_last' with NCHW strides, its freshly allocated gradient is not)."""
    return a.shape == b.shape and all(sa == sb for sa, sb, n in zip(a.stride(), b.stride(), a.shape) if n > 1)


def _chunk_rows(p, g, m, v):
    """The records {p, g, m, v, n} of one tensor for the multi-tensor kernels: CHUNK elements each, the last one the rest."""
    ptrs = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr())
    n = p.numel()
    return [(ptrs[0] + 4 * off, ptrs[1] + 4 * off, ptrs[2] + 4 * off, ptrs[3] + 4 * off, min(CHUNK, n - off))
            for off in range(0, n, CHUNK)]


class _FusedOptimizer(torch.optim.Optimizer):
    """What Adam and AdamW share: the moments' creation, the loader of a stock optimiser's state, which tensors of a group can
    go through one multi-tensor launch, and the upload of the pointer table."""

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._pin_rings = {}          # (group, table size) -> [[pinned int64 buffer, event of its last upload], ...]

    def load_state_dict(self, state_dict):
        """Accepts the state a stock torch.optim.Adam / AdamW saved (for the reference: a Lightning checkpoint's
        `optimizer_states`): its moments keep the NCHW strides they were saved with and `step` is a tensor; both are brought
        to this optimiser's conventions (moments in the parameter's own - channels_last - layout, integer step)."""
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p)
                if not st:
                    continue
                if torch.is_tensor(st.get("step")):
                    st["step"] = int(st["step"].item())
                for k in ("exp_avg", "exp_avg_sq"):
                    t = st.get(k)
                    if t is not None and not _same_layout(t, p):
                        st[k] = torch.empty_strided(p.size(), p.stride(), dtype=p.dtype, device=p.device).copy_(t)

    def _init_state(self, p):
        state = self.state[p]
        if len(state) == 0:
            state["step"] = 0
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return state

    def _multi_plan(self, group):
        """(params with a gradient, the step count they are about to take) when all of them can go through one multi-tensor
        launch, else (params, None): tensors that do not share a step count or a device, or a gradient that needs a layout
        copy, leave the group to the per-tensor path."""
        params = [p for p in group["params"] if p.grad is not None]
        if not params:
            return params, 0
        dev = params[0].device
        steps = set()
        for p in params:
            if not p.is_cuda or p.device != dev or not _same_layout(p.grad, p):
                return params, None
            state = self._init_state(p)
            if not (_same_layout(state["exp_avg"], p) and _same_layout(state["exp_avg_sq"], p)):
                return params, None
            steps.add(state["step"])
        if len(steps) != 1:
            return params, None
        return params, steps.pop() + 1

    def _layout_fixed_grad(self, p):
        """(gradient in the parameter's layout, exp_avg, exp_avg_sq) of the per-tensor path: an element-wise update works on any
        dense layout as long as p, g, m, v share it."""
        if not p.is_cuda:
            raise RuntimeError("hipops.%s needs parameters on a ROCm device" % type(self).__name__)
        g = p.grad
        state = self._init_state(p)
        if not _same_layout(g, p):
            g = torch.empty_strided(p.size(), p.stride(), dtype=p.dtype, device=p.device).copy_(p.grad)
        m, v = state["exp_avg"], state["exp_avg_sq"]
        if not (_same_layout(m, p) and _same_layout(v, p)):
            raise RuntimeError("%s state layout does not match the parameter layout" % type(self).__name__)
        return g, m, v

    def _upload_table(self, key, rows, dev):
        """The chunk rows as a device tensor (len(rows), 5) int64.  The pointer table goes up through a small ring of persistent
        pinned buffers (a fresh pinned allocation per step can make the host allocator wait for the device); a slot is reused
        only after its copy has run.  The caller record_stream()s the table after its last launch."""
        arr = np.asarray(rows, dtype=np.int64)
        ring = self._pin_rings.setdefault((key, arr.size), [])
        slot = None
        for cand in ring:
            if cand[1].query():
                slot = cand
                break
        if slot is None:
            if len(ring) >= 8:
                slot = ring[0]
                slot[1].synchronize()
            else:
                slot = [torch.empty(arr.size, dtype=torch.int64).pin_memory(), torch.cuda.Event()]
                ring.append(slot)
        slot[0].numpy()[:] = arr.reshape(-1)
        table = slot[0].to(dev, non_blocking=True).view(arr.shape)
        slot[1].record(torch.cuda.current_stream())
        return table


class Adam(_FusedOptimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = _ops._L()         # torch.ops.vqw.adam_step / adam_multi (hipops/library.py)
        for group in self.param_groups:
            b1, b2 = group["betas"]
            if MULTI_TENSOR and self._step_multi(L, group):
                continue
            for p in group["params"]:
                if p.grad is None:
                    continue
                g, m, v = self._layout_fixed_grad(p)
                state = self.state[p]
                state["step"] += 1
                t = state["step"]
                L.vqw_adam_step(p, g, m, v, p.numel(), group["lr"], b1, b2, group["eps"],
                                group["weight_decay"], 1.0 - b1 ** t, 1.0 - b2 ** t)
        _ops.bump_weight_epoch()      # parameters changed through raw pointers: invalidate derived weight layouts
        return loss

    def _step_multi(self, L, group):
        """All tensors of the group in one launch.  Falls back (returns False) when the tensors do not share a step
        count or a gradient needs a layout copy; the per-tensor path then handles the group."""
        params, t = self._multi_plan(group)
        if not params:
            return True
        if t is None:
            return False
        rows = []
        for p in params:
            state = self.state[p]
            state["step"] = t
            rows += _chunk_rows(p, p.grad, state["exp_avg"], state["exp_avg_sq"])
        table = self._upload_table(id(group), rows, params[0].device)
        b1, b2 = group["betas"]
        L.vqw_adam_multi(table, len(rows), group["lr"], b1, b2, group["eps"],
                         group["weight_decay"], 1.0 - b1 ** t, 1.0 - b2 ** t)
        table.record_stream(torch.cuda.current_stream())
        return True


class AdamW(_FusedOptimizer):
    """torch.optim.AdamW with the gradient clip inside.  Per step: one vqw_grad_norm_multi launch pair over the records of all
    groups (only with max_grad_norm), then one vqw_adamw_multi launch per group with that group's lr and weight_decay; a group
    whose tensors do not share a step count or a layout goes through vqw_adamw_step per tensor, as Adam's does.

    max_grad_norm: None or <= 0 switches the clip off.  last_grad_norm: the pre-clip global norm of the last step as a 0-dim
    device tensor (None without the clip or before the first step) - nothing here reads it; last_clip_coef likewise.  The
    gradients themselves are not scaled: p.grad keeps the unclipped values, unlike torch's in-place clip_grad_norm_."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid AdamW hyper-parameters")
        if max_grad_norm is not None and not float(max_grad_norm) == float(max_grad_norm):
            raise ValueError("invalid AdamW max_grad_norm")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.max_grad_norm = None if max_grad_norm is None or max_grad_norm <= 0 else float(max_grad_norm)
        self.last_grad_norm = None
        self.last_clip_coef = None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = _ops._L()         # torch.ops.vqw.grad_norm_multi / adamw_multi / adamw_step (hipops/library.py)
        # what every group is going to do, and the chunk rows of all of them in one table: [group, tensors, step or None, first row, rows]
        plans, rows, dev = [], [], None
        for group in self.param_groups:
            params, t = self._multi_plan(group) if MULTI_TENSOR else ([p for p in group["params"] if p.grad is not None], None)
            if not params:
                continue
            tensors = [(p, p.grad, self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"]) if t is not None
                       else (p,) + self._layout_fixed_grad(p) for p in params]
            for p, _, _, _ in tensors:
                if dev is not None and p.device != dev:
                    raise RuntimeError("hipops.AdamW needs all parameters on one device")
                dev = p.device
            first = len(rows)
            if t is not None or self.max_grad_norm is not None:
                for q in tensors:
                    rows += _chunk_rows(*q)
            plans.append((group, tensors, t, first, len(rows) - first))
        clip = None
        table = self._upload_table("all", rows, dev) if rows else None
        if self.max_grad_norm is not None and rows:
            ws = torch.empty(L.vqw_grad_norm_ws_bytes(len(rows)) // 8, dtype=torch.float64, device=dev)
            out = torch.empty(2, dtype=torch.float32, device=dev)
            L.vqw_grad_norm_multi(table, len(rows), self.max_grad_norm, ws, ws.numel() * 8, out)
            self.last_grad_norm, self.last_clip_coef = out[0], out[1]
            clip = out[1:]
        for group, tensors, t, first, count in plans:
            b1, b2 = group["betas"]
            if t is not None:
                for p, _, _, _ in tensors:
                    self.state[p]["step"] = t
                L.vqw_adamw_multi(table[first:first + count], count, group["lr"], b1, b2, group["eps"], group["weight_decay"],
                                  1.0 - b1 ** t, 1.0 - b2 ** t, clip)
                continue
            for p, g, m, v in tensors:
                state = self.state[p]
                state["step"] += 1
                t1 = state["step"]
                L.vqw_adamw_step(p, g, m, v, p.numel(), group["lr"], b1, b2, group["eps"], group["weight_decay"],
                                 1.0 - b1 ** t1, 1.0 - b2 ** t1, clip)
        if table is not None:
            table.record_stream(torch.cuda.current_stream())
        _ops.bump_weight_epoch()      # parameters changed through raw pointers: invalidate derived weight layouts
        return loss
