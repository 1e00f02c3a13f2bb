"""First training step of the VQ-W-Net (reference: trainers/single_window_trainer.py:68-147,
construction per trainers/base.py:164-237, 261-278) on the MI355X kernels.

PyTorch-Lightning and kornia are not part of this build: the trainer is a plain class that
owns the same modules, optimisers and loss weighting and exposes `training_step(batch)`.
The two augmented views are produced by a `views` callable; the default is the exact-integer
pair (identity, horizontal flip + additive noise on the noised copy) whose cross-view id
map is an index flip.
"""
from collections import namedtuple
import os

import torch

from hipops import ops, Adam
from networks import UNetEncoder, UNetDecoder
from functions import EmbeddingLoss, OneHotEncoder
from utils import norm, denorm
from .base import StepThrottle, TrainerBase  # noqa: F401  (StepThrottle: imported from here by older code)
from .data_parallel import GradientAllReducer
from . import window_terms

LossWeights = namedtuple("LossWeights", "commit cross dist reg recon freq perceptual", defaults=(1.0,) * 5 + (0.0, 0.0))


class FlipViews:
    """view 1 = identity, view 2 = horizontal flip; noise (if given) only on the noised copy of view 2.
    `cross_ids(ids, which)` maps a view's id map into the other view's frame (flip), zeroing a border."""

    def __init__(self, border=0):
        self.border = border

    def __call__(self, image, noise=None):
        flipped = torch.flip(image, dims=[3])
        noised2 = flipped if noise is None else ops.add(flipped, noise)
        return (image, image), (noised2, flipped)

    def cross_ids(self, ids, which=1):
        return ops.flip_labels(ids, self.border)


class RandomTransformViews:
    """The reference's pair of RandomTransform modules (trainers/base.py:280-282) behind the `views` protocol:
    images arrive in [-1, 1], are augmented in [0, 1] and handed back in [-1, 1] (single_window_trainer.py:73-83);
    cross_ids(ids, which) = other.forward_transform(own.reverse_transform(ids)) (:91-96)."""

    def __init__(self, transform_1, transform_2):
        self.t = (transform_1, transform_2)

    def __call__(self, image, noise=None):
        x = denorm(image.clone(), vmin=0, vmax=1)           # norm / denorm work in place: keep the batch intact
        n1, c1 = self.t[0](x.clone())
        n2, c2 = self.t[1](x)
        return (norm(n1), norm(c1)), (norm(n2), norm(c2))

    def cross_ids(self, ids, which=1):
        own, other = (self.t[0], self.t[1]) if which == 1 else (self.t[1], self.t[0])
        return other.forward_transform(own.reverse_transform(ids))

    def state_dict(self):
        """The two host generators the augmentation parameters are drawn from."""
        return {"generators": [t.generator.get_state() for t in self.t]}

    def load_state_dict(self, state):
        for t, g in zip(self.t, state["generators"]):
            t.generator.set_state(g)


trainer_state_dict = TrainerBase.state_dict              # (trainer) and (trainer, state), for anything that has modules()
load_trainer_state_dict = TrainerBase.load_state_dict    # and optimizers(): the names these had as functions of this module


LUNG_WINDOW, MEDIASTINAL_WINDOW = window_terms.LUNG_WINDOW, window_terms.MEDIASTINAL_WINDOW    # the names they have here


class FirstStepTrainer(TrainerBase):
    def __init__(self, in_channels=1, enc_filters=(16, 32, 64, 128, 256), dec_filters=(32, 64, 128, 256, 512),
                 dict_size=10, momentum=0.999, margin=0.5, loss_weight=None, lr=1e-4, betas=(0.5, 0.999),
                 weight_decay=0.0, use_pixel_shuffle=False, dropped_skip_layers=(), views=None, device="cuda",
                 encoder=None, decoder=None, data_parallel=False, use_onehot=False, concurrent_views=None,
                 multi_window=None, embed_loss=None, enc_optim=None, dec_optim=None, use_recon_loss=True,
                 frequency_loss=None, freq_weights=None, perceptual_loss=None, percep_weights=None):
        super().__init__(device)
        self.encoder = encoder if encoder is not None else UNetEncoder(
            in_channels, list(enc_filters), dict_size, momentum, 'torch', False, 1, True)
        self.decoder = decoder if decoder is not None else UNetDecoder(
            enc_filters[0], in_channels, list(dec_filters), use_dropblock=False,
            dropped_skip_layers=list(dropped_skip_layers), use_styled_up_block=True, use_pixel_shuffle=use_pixel_shuffle)
        self.encoder.to(self.device).train()
        self.decoder.to(self.device).train()
        self.dict_size = dict_size
        self.embed_loss = embed_loss if embed_loss is not None else EmbeddingLoss(dict_size, margin, True, True)
        self.use_recon_loss = bool(use_recon_loss)       # config.loss.use_recon_loss (single_window_trainer.py:110-115)
        self.one_hot_encoder = OneHotEncoder(n_classes=dict_size + 1)
        self.use_onehot = use_onehot
        self.w = loss_weight if loss_weight is not None else LossWeights()
        self.views = views if views is not None else FlipViews()
        # multi_window = dict(dataset_window=(width, center, scale), recon_weights=(w_full, w_lung, w_mediastinal)): the
        # reconstruction term of trainers/multi_window_trainer.py:93-118 (same step otherwise)
        self.multi_window = multi_window
        # frequency_loss: functions.FocalFrequencyLoss (config.loss.use_frequency_loss) or None; in multi-window runs
        # freq_weights = config.loss.freq_weights (w_full, w_lung, w_mediastinal), multi_window_trainer.py:100-126
        self.frequency_loss = frequency_loss
        self.freq_weights = tuple(freq_weights) if freq_weights is not None else None
        if frequency_loss is not None and multi_window is not None and self.freq_weights is None:
            raise ValueError("multi-window training with the frequency loss needs freq_weights (config.loss.freq_weights)")
        # perceptual_loss: functions.VGGLoss (config.loss.use_perceptual_loss) or None; in multi-window runs
        # percep_weights = config.loss.percep_weights (w_full, w_lung, w_mediastinal), multi_window_trainer.py:54, 101-119
        self.perceptual_loss = perceptual_loss.to(self.device) if perceptual_loss is not None else None
        self.percep_weights = tuple(percep_weights) if percep_weights is not None else None
        if perceptual_loss is not None and multi_window is not None and self.percep_weights is None:
            raise ValueError("multi-window training with the perceptual loss needs percep_weights (config.loss.percep_weights)")
        # base.py:165-175: one Adam per sub-network over its trainable parameters
        # (enc_optim / dec_optim: dicts with lr, betas, weight_decay per sub-network, as config.enc_optim / dec_optim give)
        eo = {**dict(lr=lr, betas=betas, weight_decay=weight_decay), **(enc_optim or {})}
        do = {**dict(lr=lr, betas=betas, weight_decay=weight_decay), **(dec_optim or {})}
        self.enc_optim = Adam([p for p in self.encoder.parameters() if p.requires_grad], **eo)
        self.dec_optim = Adam([p for p in self.decoder.parameters() if p.requires_grad], **do)
        # the two views are independent chains (coupled only through in-order VQ / BN buffer updates, which the ops
        # order with events): running them on two streams lets HBM-bound kernels of one overlap MFMA-bound kernels of
        # the other.  VQW_CONCURRENT_VIEWS=0/1 overrides the default.
        if concurrent_views is None:
            concurrent_views = os.environ.get("VQW_CONCURRENT_VIEWS", "1") != "0"
        self.concurrent_views = bool(concurrent_views) and self.device.type == "cuda"
        self._s2 = None
        self.reducer = None
        self._params = list(self.encoder.parameters()) + list(self.decoder.parameters())
        if data_parallel:
            params = [p for p in self.decoder.parameters() if p.requires_grad][::-1] + \
                     [p for p in self.encoder.parameters() if p.requires_grad][::-1]
            self.reducer = GradientAllReducer(params)      # buckets in backward order: decoder tail first

    def _forward_losses_two_streams(self, image, noise):
        """Same arithmetic as forward_losses; view 1 on the current stream, view 2 on a second stream."""
        s1 = torch.cuda.current_stream()
        if self._s2 is None:
            self._s2 = torch.cuda.Stream(device=self.device, priority=-1)
        s2 = self._s2
        (noised_1, clear_1), (noised_2, clear_2) = self.views(image, noise)
        s2.wait_event(s1.record_event())
        for t in (noised_2, clear_2):
            t.record_stream(s2)
        with torch.cuda.stream(s2):
            feat_2 = self.encoder.feature_extraction(noised_2)
        embed_1, l_commit_1, ids_1 = self.encoder(noised_1)
        r_ids_1 = self.views.cross_ids(ids_1, 1)
        ev1 = s1.record_event()
        with torch.cuda.stream(s2):
            embed_2, l_commit_2, ids_2 = self.encoder.vq(feat_2, id_base=1)       # ordered after view 1's update
            ids_2 = torch.transpose(ids_2, 1, 2)
            r_ids_2 = self.views.cross_ids(ids_2, 2)
            # The embedding loss runs on view 2's stream.  Autograd replays a node on the stream of its forward and in
            # reverse creation order: on stream 1 the loss's (tiny) backward would queue behind ALL of view 1's decoder
            # backward, and view 2's encoder backward, which needs its gradient, would start only then (stream 2 idle
            # for the last fifth of the step).  On stream 2 it follows view 2's decoder backward directly.
            s2.wait_event(ev1)
            for t in (embed_1, r_ids_1):
                t.record_stream(s2)
            codebook = self.encoder.vq.get_codebook()
            l_cross, l_dist, l_reg = self.embed_loss.forward_labels(embed_1, r_ids_1, embed_2, r_ids_2, codebook)
        recon_1 = self.decoder(embed_1)
        terms_1 = self._view_terms(recon_1, clear_1)
        with torch.cuda.stream(s2):
            recon_2 = self.decoder(embed_2)
            terms_2 = self._view_terms(recon_2, clear_2)
            ev2 = s2.record_event()
        s1.wait_event(ev2)
        for t in [l_commit_2, recon_2, l_cross, embed_2, r_ids_2, ids_2] + [t for part in terms_2 for t, _ in part] + \
                [t for t in (l_dist, l_reg) if torch.is_tensor(t)]:
            t.record_stream(s1)
        return self._assemble(l_commit_1, l_commit_2, l_cross, l_dist, l_reg, terms_1, terms_2, (ids_1, ids_2),
                              (recon_1, recon_2), (embed_1, embed_2))

    def _assemble(self, l_commit_1, l_commit_2, l_cross, l_dist, l_reg, terms_1, terms_2, ids, recons, embeds):
        """The total and the returned dict of either forward path.  terms_i: view i's (reconstruction, frequency, perceptual)
        lists of (loss term, weight).  ops.weighted_sum adds in the order given, so the order is part of the total's bits."""
        w = self.w
        (rec_1, frq_1, pcp_1), (rec_2, frq_2, pcp_2) = terms_1, terms_2
        terms = rec_1 + rec_2 + frq_1 + frq_2 + pcp_1 + pcp_2
        l_total = ops.weighted_sum(
            [l_commit_1, l_commit_2, l_cross, l_dist, l_reg] + [t for t, _ in terms],
            [w.commit, w.commit, w.cross, w.dist, w.reg] + [c for _, c in terms])
        out = dict(total=l_total, commit_1=l_commit_1, commit_2=l_commit_2, cross=l_cross, dist=l_dist, reg=l_reg,
                   recon_l1=rec_1[0][0], recon_l2=rec_2[0][0], ids_1=ids[0], ids_2=ids[1], recon_1=recons[0], recon_2=recons[1],
                   embed_1=embeds[0], embed_2=embeds[1])
        if frq_1:                 # only with the frequency loss on: without it the step returns what it always did
            out.update(freq_1=frq_1[0][0], freq_2=frq_2[0][0])
        if pcp_1:                 # likewise only with the perceptual loss on
            out.update(perceptual_1=pcp_1[0][0], perceptual_2=pcp_2[0][0])
        return out

    def _view_terms(self, recon, clear):
        """One view's (reconstruction, frequency, perceptual) term lists."""
        return self._recon_terms(recon, clear), self._freq_terms(recon, clear), self._percep_terms(recon, clear)

    def _recon_terms(self, recon, clear):
        """[(loss term, weight)] of one view's reconstruction loss (window_terms.recon_terms)."""
        if not self.use_recon_loss:          # l_recon = 0.0 upstream: the term is still reported, with weight zero
            return [(ops.mse_loss(recon.detach(), clear), 0.0)]
        return window_terms.recon_terms(recon, clear, self.multi_window, self.w.recon)

    def _freq_terms(self, recon, clear):
        """[(loss term, weight)] of one view's focal frequency loss (window_terms.freq_terms)."""
        return window_terms.freq_terms(self.frequency_loss, recon, clear, self.multi_window, self.freq_weights, self.w.freq)

    def _percep_terms(self, recon, clear):
        """[(loss term, weight)] of one view's perceptual loss (window_terms.percep_terms)."""
        return window_terms.percep_terms(self.perceptual_loss, recon, clear, self.multi_window, self.percep_weights,
                                         self.w.perceptual)

    def forward_losses(self, image, noise=None):
        """Lines 73-137 of the reference step.  `image` is in [-1, 1] (dataloader convention)."""
        if self.concurrent_views and not self.use_onehot:
            return self._forward_losses_two_streams(image, noise)
        (noised_1, clear_1), (noised_2, clear_2) = self.views(image, noise)
        embed_1, l_commit_1, ids_1 = self.encoder(noised_1)
        embed_2, l_commit_2, ids_2 = self.encoder(noised_2)
        r_ids_1 = self.views.cross_ids(ids_1, 1)
        r_ids_2 = self.views.cross_ids(ids_2, 2)
        codebook = self.encoder.vq.get_codebook()
        if self.use_onehot:      # the reference's literal route: (B,K+1,H,W) one-hot, class 0 dropped
            oh1 = self.one_hot_encoder(r_ids_1)[:, 1:, ...]
            oh2 = self.one_hot_encoder(r_ids_2)[:, 1:, ...]
            l_cross, l_dist, l_reg = self.embed_loss(embed_1, oh1, embed_2, oh2, codebook)
        else:
            l_cross, l_dist, l_reg = self.embed_loss.forward_labels(embed_1, r_ids_1, embed_2, r_ids_2, codebook)
        recon_1 = self.decoder(embed_1)
        recon_2 = self.decoder(embed_2)
        rec_1, rec_2 = self._recon_terms(recon_1, clear_1), self._recon_terms(recon_2, clear_2)
        frq_1, frq_2 = self._freq_terms(recon_1, clear_1), self._freq_terms(recon_2, clear_2)
        pcp_1, pcp_2 = self._percep_terms(recon_1, clear_1), self._percep_terms(recon_2, clear_2)
        return self._assemble(l_commit_1, l_commit_2, l_cross, l_dist, l_reg, (rec_1, frq_1, pcp_1), (rec_2, frq_2, pcp_2),
                              (ids_1, ids_2), (recon_1, recon_2), (embed_1, embed_2))

    # `modules` / `optimizers` are in the reference's order
    def modules(self):
        return {"encoder": self.encoder, "decoder": self.decoder}

    def optimizers(self):
        return {"enc": self.enc_optim, "dec": self.dec_optim}

    def _join(self):
        """After the backward pass: the second view's stream back into the current one, then the end of the ops' step."""
        if self._s2 is not None:
            torch.cuda.current_stream().wait_stream(self._s2)
        ops.join_streams()

    def training_step(self, batch, noise=None, mark=None):
        """`mark(name)`, if given, is called at the end of each phase: 'begin', 'forward', those of TrainerBase.update, 'end'."""
        image = batch['image'] if isinstance(batch, dict) else batch
        self.throttle.begin()
        ops.begin_step()
        if self.reducer is not None:
            ops.reset_pending(self._params)
        if mark is not None:
            mark("begin")
        out = self.forward_losses(image, noise)
        if mark is not None:
            mark("forward")
        self.update(out["total"], [self.enc_optim, self.dec_optim], self.reducer, self._join, mark)
        self.throttle.end()
        if mark is not None:
            mark("end")
        return out

    @staticmethod
    def scalars(out):
        """Host copies of the logged scalars (one sync; keep out of timed regions); `freq` is 0.0 without the frequency loss,
        `perceptual` is there only with the perceptual loss on."""
        f = lambda t: float(t.detach()) if torch.is_tensor(t) else float(t)  # noqa: E731
        sc = dict(total=f(out["total"]), commit=f(out["commit_1"]) + f(out["commit_2"]), cross=f(out["cross"]),
                  dist=f(out["dist"]), reg=f(out["reg"]), recon=f(out["recon_l1"]) + f(out["recon_l2"]),
                  freq=f(out.get("freq_1", 0.0)) + f(out.get("freq_2", 0.0)))
        if "perceptual_1" in out:
            sc["perceptual"] = f(out["perceptual_1"]) + f(out["perceptual_2"])
        return sc
