"""Host tests of trainers.base.TrainerBase.update, the one optimiser update every training step goes through: each site's
sequence, with recording stand-ins for optimisers, reducer and loss (no GPU)."""
import torch


class _Recorder:
    """Stands in for an optimiser, a reducer or a loss: every call is appended to `log` as '<name>.<method>'."""

    def __init__(self, log, name):
        self.log, self.name = log, name

    def __getattr__(self, method):
        if method.startswith("__"):
            raise AttributeError(method)
        return lambda *a, **k: self.log.append("%s.%s" % (self.name, method))


def _stand_ins():
    log = []
    return log, {n: _Recorder(log, n) for n in ("enc", "dec", "dis", "reducer", "loss")}, lambda name: log.append("mark:" + name)


def test_update_first_step_sequence():
    """Both zero_grads before prepare; the post-backward action after backward; finish after it and before either step; `mark`
    at every phase boundary."""
    from trainers.base import TrainerBase
    log, s, mark = _stand_ins()
    TrainerBase.update(s["loss"], [s["enc"], s["dec"]], s["reducer"], lambda: log.append("join"), mark)
    assert log == ["enc.zero_grad", "dec.zero_grad", "reducer.prepare", "mark:zero+prepare", "loss.backward", "mark:backward",
                   "join", "mark:join", "reducer.finish", "mark:finish", "enc.step", "dec.step", "mark:optim"]
    # the same without a reducer and without marks: what a single-GPU training run executes
    del log[:]
    TrainerBase.update(s["loss"], [s["enc"], s["dec"]], None, lambda: log.append("join"))
    assert log == ["enc.zero_grad", "dec.zero_grad", "loss.backward", "join", "enc.step", "dec.step"]


def test_update_discriminator_sequence_has_no_post_backward_action():
    from trainers.base import TrainerBase
    log, s, mark = _stand_ins()
    TrainerBase.update(s["loss"], [s["dis"]], s["reducer"], mark=mark)
    assert log == ["dis.zero_grad", "reducer.prepare", "mark:zero+prepare", "loss.backward", "mark:backward", "reducer.finish",
                   "mark:finish", "dis.step", "mark:optim"]
    del log[:]
    TrainerBase.update(s["loss"], [s["dis"]])
    assert log == ["dis.zero_grad", "loss.backward", "dis.step"]


def test_first_step_training_step_goes_through_update(monkeypatch):
    """FirstStepTrainer.training_step itself, forward stubbed: begin_step before the forward, then the first-step sequence with
    ops.join_streams() as the post-backward action, the throttle around all of it."""
    from hipops import ops
    from trainers import FirstStepTrainer
    log, s, mark = _stand_ins()
    monkeypatch.setattr(ops, "begin_step", lambda: log.append("ops.begin_step"))
    monkeypatch.setattr(ops, "join_streams", lambda: log.append("ops.join_streams"))
    monkeypatch.setattr(ops, "reset_pending", lambda params: log.append("ops.reset_pending"))
    tr = object.__new__(FirstStepTrainer)
    tr.throttle, tr.enc_optim, tr.dec_optim, tr.reducer = _Recorder(log, "throttle"), s["enc"], s["dec"], s["reducer"]
    tr._s2, tr._params = None, []
    out = {"total": s["loss"]}
    tr.forward_losses = lambda image, noise: log.append("forward") or out
    assert tr.training_step({"image": torch.zeros(1)}, mark=mark) is out
    assert log == ["throttle.begin", "ops.begin_step", "ops.reset_pending", "mark:begin", "forward", "mark:forward",
                   "enc.zero_grad", "dec.zero_grad", "reducer.prepare", "mark:zero+prepare", "loss.backward", "mark:backward",
                   "ops.join_streams", "mark:join", "reducer.finish", "mark:finish", "enc.step", "dec.step", "mark:optim",
                   "throttle.end", "mark:end"]
