"""What every trainer of this package shares: the step throttle, what a run saves and restores, the test step, and the
one optimiser update (zero_grad -> reducer.prepare -> backward -> ... -> reducer.finish -> step) all training steps go through.
"""
import collections
import os

import torch

from .evaluation import Evaluator


class StepThrottle:
    """At most `max_inflight` training steps enqueued ahead of the GPU (VQW_MAX_INFLIGHT, default 2).

    The host enqueues a step five times faster than the GPU runs it.  Unthrottled it gets many steps ahead, and every
    tensor that was handed to another stream (record_stream: conv inputs / gradients used by the weight-gradient lanes,
    the second view) cannot be reused by the caching allocator until the GPU has passed its last use: the allocator
    then hipMallocs a fresh working set for every step in flight (+10 GB of reserved memory per step measured, with
    sporadic stalls of 0.3-1 s in those calls).  Two steps in flight keep the GPU fed and the pool bounded."""

    def __init__(self, device):
        self.cuda = torch.device(device).type == "cuda"
        self.events = collections.deque()
        self.max_inflight = max(1, int(os.environ.get("VQW_MAX_INFLIGHT", "2")))

    def begin(self):
        while len(self.events) >= self.max_inflight:
            self.events.popleft().synchronize()

    def end(self):
        if self.cuda:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            self.events.append(ev)


class TrainerBase:
    """A subclass supplies modules() and optimizers() ({name: module / optimiser}, in the reference's order, with a
    'decoder' and - every trainer but the VQGAN's, whose 'decoder' is the whole autoencoder - an 'encoder' among the modules)
    and sets `dict_size`."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.throttle = StepThrottle(self.device)      # at most two steps enqueued ahead of the GPU

    def modules(self):
        raise NotImplementedError

    def optimizers(self):
        raise NotImplementedError

    # -- what a run saves and restores (trainers/fit.py)
    def state_dict(self):
        """{'modules': {name: state_dict}, 'optimizers': {name: state_dict}, 'extra': ...}.  `extra` is what the module and
        optimiser state dicts do not hold and a bit-exact continuation needs: the views' generators, the DropBlock
        schedule's position and the encoder's codebook-initialised flag."""
        mods = self.modules()
        extra = {}
        if "encoder" in mods:
            extra["init_embed"] = bool(mods["encoder"].init_embed)
        views = getattr(self, "views", None)
        if hasattr(views, "state_dict"):
            extra["views"] = views.state_dict()
        sched = getattr(mods["decoder"], "dropblock", None)
        if hasattr(sched, "drop_values"):
            extra["dropblock"] = {"i": int(sched.i), "drop_prob": float(sched.dropblock.drop_prob)}
        return {"modules": {k: m.state_dict() for k, m in mods.items()},
                "optimizers": {k: o.state_dict() for k, o in self.optimizers().items()}, "extra": extra}

    def load_state_dict(self, state):
        mods = self.modules()
        for k, m in mods.items():
            if k in state.get("modules", {}):
                m.load_state_dict(state["modules"][k], strict=True)
        for k, o in self.optimizers().items():
            if k in state.get("optimizers", {}):
                o.load_state_dict(state["optimizers"][k])
        extra = state.get("extra") or {}
        if "init_embed" in extra and "encoder" in mods:
            mods["encoder"].init_embed = bool(extra["init_embed"])
        views = getattr(self, "views", None)
        if "views" in extra and hasattr(views, "load_state_dict"):
            views.load_state_dict(extra["views"])
        sched = getattr(mods["decoder"], "dropblock", None)
        if "dropblock" in extra and hasattr(sched, "drop_values"):
            sched.i = int(extra["dropblock"]["i"])
            sched.dropblock.drop_prob = extra["dropblock"]["drop_prob"]

    def test_step(self, batch):
        """The reference's test step (single_window_trainer.py:781-827): {'NMSE', 'SSIM', 'PSNR', 'Entropy'} of one batch
        through trainers.evaluation.Evaluator (eval mode, no gradients; training state untouched)."""
        mods = self.modules()
        if "encoder" not in mods:
            raise NotImplementedError("%s has no test step (the reference defines none for it)" % type(self).__name__)
        return Evaluator(mods["encoder"], mods["decoder"], self.dict_size).test_step(batch)

    @staticmethod
    def update(loss, optims, reducer=None, after_backward=None, mark=None):
        """One update of `optims` on `loss`: zero their gradients, reducer.prepare(), loss.backward(), after_backward() (what
        has to follow the backward pass before gradients are final: stream joins), reducer.finish(), the optimiser steps.
        `mark(name)`, if given, is called at the end of each of these phases (the timing tools: tools/step_phases.py)."""
        for o in optims:
            o.zero_grad()
        if reducer is not None:
            reducer.prepare()
        if mark is not None:
            mark("zero+prepare")
        loss.backward()
        if mark is not None:
            mark("backward")
        if after_backward is not None:
            after_backward()
            if mark is not None:
                mark("join")
        if reducer is not None:
            reducer.finish()
        if mark is not None:
            mark("finish")
        for o in optims:
            o.step()
        if mark is not None:
            mark("optim")
