"""Test-mode evaluation (`run_vqwnet.py -m test`): the reference's SingleWindowTrainer._test_step / _test_epoch_end
(trainers/single_window_trainer.py:54-66, 781-848).

Per batch, in eval mode and without gradients: embed, _, ids = encoder(image); recon = decoder(embed); then
NMSE (torchmetrics MeanSquaredError: plain MSE despite the key), SSIM, PSNR (torchmetrics 0.6.2 defaults, the batch's own
values) and Entropy (base-2 entropy of the counts of ids 1..K) from one call of the HIP metric kernels
(hipops.ops.recon_metrics_values: four launches, one device-to-host read).  At the end of the epoch the mean and the
population std over batches of each key go to `result.csv` in pandas.DataFrame.to_csv layout.

Deviations from the reference: no PNGs are written, and every dataset is scored (the reference saves PNGs and raises
NotImplementedError for every dataset but CRC, :803-823).  As there, only rank 0 scores: with a process group up the other
ranks return None.
"""
import csv
import math
import os

import numpy as np
import torch
import torch.distributed as dist

from hipops import ops

KEYS = ("NMSE", "SSIM", "PSNR", "Entropy")


def _is_rank_zero():
    return not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0


def _csv_float(v):
    """A float as pandas.DataFrame.to_csv writes it: the shortest round-trip repr, nan as an empty field."""
    v = float(v)
    return "" if math.isnan(v) else repr(v)


def write_result_csv(result, path):
    """result: {column: value} -> `path` as pandas.DataFrame.from_dict({k: [v]}).to_csv(path) writes it."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow([""] + list(result))
        w.writerow(["0"] + [_csv_float(v) for v in result.values()])


class Evaluator:
    def __init__(self, encoder, decoder, dict_size, keep_outputs=False):
        self.encoder = encoder
        self.decoder = decoder
        self.dict_size = int(dict_size)
        self.keep_outputs = keep_outputs      # keep the last batch's (image, recon, ids) in self.last (inspection, tests)
        self.last = None

    @torch.no_grad()
    def test_step(self, batch):
        """-> {'NMSE', 'SSIM', 'PSNR', 'Entropy'} as Python floats (None on ranks other than 0).  The networks run in eval
        mode (the forward-only path run_recon takes) and get their previous modes back afterwards."""
        if not _is_rank_zero():
            return None
        image = batch["image"] if isinstance(batch, dict) else batch
        device = next(self.encoder.parameters()).device
        image = image.to(device, non_blocking=True)
        modes = (self.encoder.training, self.decoder.training)
        self.encoder.eval()
        self.decoder.eval()
        try:
            embed, _, ids = self.encoder(image)
            recon = self.decoder(embed)
        finally:
            self.encoder.train(modes[0])
            self.decoder.train(modes[1])
        v = ops.recon_metrics_values(recon, image, ids, self.dict_size)
        if self.keep_outputs:
            self.last = dict(image=image, recon=recon, ids=ids)
        return dict(zip(KEYS, (v["mse"], v["ssim"], v["psnr"], v["entropy"])))

    def test_epoch_end(self, outputs, save_dir):
        """outputs: the test_step results -> {key_avg: mean, key_std: population std} in the order NMSE, SSIM, PSNR,
        Entropy, also written to save_dir/result.csv (None on ranks other than 0)."""
        if not _is_rank_zero():
            return None
        outputs = [o for o in outputs if o is not None]
        if not outputs:
            raise ValueError("test_epoch_end: no test_step outputs")
        result = {}
        for key in outputs[0]:
            values = np.asarray([o[key] for o in outputs], dtype=np.float64)
            result[key + "_avg"] = float(np.mean(values))
            result[key + "_std"] = float(np.std(values))
        os.makedirs(save_dir, exist_ok=True)
        write_result_csv(result, os.path.join(save_dir, "result.csv"))
        return result

    def run(self, loader, save_dir):
        """test_step over every batch of `loader`, then test_epoch_end -> the result dict."""
        return self.test_epoch_end([self.test_step(b) for b in loader], save_dir)
