"""Run directory, `log.csv`, saved hyper-parameters and checkpoint pruning of a training run (reference:
utils/logger.py:39-91 ModelSaver, :94-255 Logger), without PyTorch-Lightning, fsspec or the Slack uploader.

    <save_dir>/<name>/version_<n>/        n = highest existing version + 1 (0 in a fresh directory)
        config.json                       the config's sections, `seed_list` (one seed per rank) and `save_dir_path`
        log.csv                           header = monitoring_metrics; one row per logged step
        ckpt-epoch=<epoch:04d>-total_loss=0.00.ckpt
"""
import collections
import json
import os

import torch

CKPT_PREFIX = "ckpt-epoch="


def checkpoint_name(epoch):
    """The file name Lightning forms from the reference's `ckpt-{epoch:04d}-{total_loss:.2f}` (total_loss is not a logged
    metric there, so the field is always 0.00); prune_checkpoints parses the epoch back out of it."""
    return "%s%04d-total_loss=0.00.ckpt" % (CKPT_PREFIX, int(epoch))


def prune_checkpoints(dirpath, limit_num=10, save_interval=10):
    """ModelSaver._delete_old_checkpoint: of the sorted checkpoint names, all but the newest `limit_num` are deleted unless
    (epoch + 1) % save_interval == 0.  -> the deleted names."""
    names = sorted(c for c in os.listdir(dirpath) if "ckpt-epoch" in c)
    deleted = []
    if len(names) > limit_num:
        for name in names[:len(names) - limit_num]:
            epoch = int(name[len(CKPT_PREFIX):len(CKPT_PREFIX) + 4])
            if (epoch + 1) % save_interval != 0:
                os.remove(os.path.join(dirpath, name))
                deleted.append(name)
    return deleted


def _plain(v):
    """A config value (nested namedtuples from utils.load_json) as JSON-serialisable data."""
    if hasattr(v, "_asdict"):
        return {k: _plain(x) for k, x in v._asdict().items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


class Logger:
    def __init__(self, save_dir, config, monitoring_metrics, name="default", version=None):
        self._save_dir = save_dir
        self._name = name or ""
        self._config = config
        self._version = version
        self._monitoring_metrics = list(monitoring_metrics)

    @property
    def save_dir(self):
        return self._save_dir

    @property
    def name(self):
        return self._name

    @property
    def monitoring_metrics(self):
        return self._monitoring_metrics

    @property
    def root_dir(self):
        return os.path.join(self._save_dir, self._name) if self._name else self._save_dir

    @property
    def version(self):
        if self._version is None:
            self._version = self._get_next_version()
        return self._version

    @property
    def log_dir(self):
        version = self.version if isinstance(self.version, str) else "version_%d" % self.version
        return os.path.expanduser(os.path.expandvars(os.path.join(self.root_dir, version)))

    def _get_next_version(self):
        try:
            entries = os.listdir(self.root_dir)
        except OSError:
            return 0
        versions = [int(e.split("_")[1]) for e in entries
                    if e.startswith("version_") and os.path.isdir(os.path.join(self.root_dir, e)) and e.split("_")[1].isdigit()]
        return max(versions) + 1 if versions else 0

    def log_metrics(self, metrics):
        """One row of log.csv: str(value) per monitored key (a tensor: str(v.sum().item())), an empty field for a key the
        step did not produce."""
        values = []
        for key in self._monitoring_metrics:
            if key in metrics:
                v = metrics[key]
                v = str(v.sum().item()) if isinstance(v, torch.Tensor) else str(v)
            else:
                v = ""
            values.append(v)
        os.makedirs(self.log_dir, exist_ok=True)
        with open(os.path.join(self.log_dir, "log.csv"), "a") as f:
            if f.tell() == 0:
                print(",".join(self._monitoring_metrics), file=f)
            print(",".join(values), file=f)

    def log_hyperparams(self, seed_list):
        out = collections.OrderedDict()
        for key, child in self._config._asdict().items():
            out[key] = _plain(child)
        out["seed_list"] = list(seed_list)
        out["save_dir_path"] = self.log_dir
        os.makedirs(self.log_dir, exist_ok=True)
        with open(os.path.join(self.log_dir, "config.json"), "w") as f:
            json.dump(out, f, ensure_ascii=False, indent=2, sort_keys=False, separators=(",", ": "))
