"""The condition of a conditional code prior (trainers/cond_prior.py): a label map becomes one conditioning token per latent cell
and the tokens are embedded by a table of their own - taming-transformers' recipe for a segmentation-conditioned transformer,
restated.  The table lives outside the GPT, whose state_dict keys stay the reference's; the embedded tokens go in front of the
code sequence through the GPT's `embeddings=` prefix.

Classifier-free guidance (null_token=True): the table has one more row, the null embedding at null_index = n_labels, the
condition of "no label given".  Training drops the condition of whole samples onto it (forward(tokens, drop=(p, seed, call)):
ops.embedding_lookup_drop, counter-based, nothing stored) and sampling runs null_prefix(B) beside the label's prefix
(GPT.generate_masked's guided route).
"""
import torch
import torch.nn as nn

from hipops import ops


class LabelCondition(nn.Module):
    """tokens(label): (B, H, W) or (B, 1, H, W) integer label map -> (B, h w) torch.long in raster order, ops.cell_labels (the
    majority label of each cell; -1 for a cell with no pixel in [0, n_labels)).  forward(tokens): (B, h w) -> (B, h w, n_embed),
    ops.embedding_lookup in `embed.weight` (n_labels, n_embed), the module's one parameter, drawn N(0, 0.02) like the GPT's.

    null_token=True: `embed.weight` is (n_labels + 1, n_embed), its last row the null embedding (null_index = n_labels; drawn
    with the others); a label token never reaches it: ops.cell_labels gives [0, n_labels) or -1.  null_prefix(B): (B, h w,
    n_embed) of that row.  forward(tokens, drop=(p, seed, call)): the lookup with whole samples dropped onto the null row with
    probability p under (seed, call).  null_token=False: the module as it was - the same parameter shape, the same draws."""

    def __init__(self, n_labels, n_embed, h, w, null_token=False):
        super().__init__()
        n_labels, n_embed, h, w = int(n_labels), int(n_embed), int(h), int(w)
        if not 1 <= n_labels <= 256:
            raise ValueError("LabelCondition: n_labels=%d must lie in [1, 256]" % n_labels)
        if n_embed < 4 or n_embed % 4:
            raise ValueError("LabelCondition: n_embed=%d must be a positive multiple of 4" % n_embed)
        if h < 1 or w < 1:
            raise ValueError("LabelCondition: the latent grid h=%d, w=%d must be positive" % (h, w))
        self.n_labels, self.n_embed, self.h, self.w = n_labels, n_embed, h, w
        self.null_index = n_labels if null_token else None
        self.embed = nn.Embedding(n_labels + (1 if null_token else 0), n_embed)
        nn.init.normal_(self.embed.weight, mean=0.0, std=0.02)

    @torch.no_grad()
    def tokens(self, label):
        return ops.cell_labels(label, self.h, self.w, self.n_labels).reshape(label.shape[0], self.h * self.w)

    def _need_null(self, what):
        if self.null_index is None:
            raise ValueError("LabelCondition: %s needs the null embedding: build the condition with null_token=True "
                             "(model.prior.cond.null_token)" % what)

    def null_prefix(self, B):
        """(B, h w, n_embed): the null embedding at every conditioning position, through the same lookup (a gradient reaches it)."""
        self._need_null("null_prefix")
        idx = torch.full((int(B), self.h * self.w), self.null_index, dtype=torch.long, device=self.embed.weight.device)
        return ops.embedding_lookup(idx, self.embed.weight)

    def forward(self, tokens, drop=None):
        if tokens.dim() != 2 or tokens.shape[1] != self.h * self.w:
            raise ValueError("LabelCondition: tokens (B, h w) = (B, %d) expected, got %s" % (self.h * self.w, tuple(tokens.shape)))
        if drop is None:
            return ops.embedding_lookup(tokens, self.embed.weight)
        self._need_null("drop=(p, seed, call)")
        p, seed, call = drop
        return ops.embedding_lookup_drop(tokens, self.embed.weight, self.null_index, p, seed, call)
