#!/usr/bin/env python3
"""The seamless composite on one GPU, DESIGN 6z9's protocol: N = 4 slices of 512 x 512, one channel, a 16 x 16 cell grid (cells of
32 x 32 pixels) with the central quarter of the cells set - configs/prior_vqgan_512_edit.json's box.

blend_cells   ops.blend_cells at levels 3 and 5, sources 'edit' (d = edit - image) and 'delta' (d = edit - recon), beside
              ops.paste_cells (the hard paste it replaces) and beside the plain-torch restatement on the same GPU: F.conv2d with the
              5 x 5 kernel and stride 2 over a replicate-padded input for REDUCE, the two-phase (even / odd) EXPAND, fp32.  Launches
              per call: 2 levels (levels reduces, levels collapses; no fused tail).  floor_bytes: the pictures read twice, out written
              once, and the workspace written and read once.
seams         from the float64 restatement (tests/blend_ref.py) on synthetic slices: the largest |difference| between neighbouring
              pixels on the two sides of the region's boundary - of the slice itself, of the hard paste and of the blend at
              levels 1..5, for both sources; each for the composite and for composite - slice (what the edit added: the slice's own
              texture taken out).  The stand-ins for the two decodes: recon = the slice through one REDUCE and EXPAND (the first
              stage's blur) plus a bias of 0.05; edit = recon (`same_codes`: the prior redrew the codes the slice had) or recon plus a
              smooth disc inside the region (`lesion`).
Per timing record: the median of --windows windows of --launches calls each, after a warm-up, the sides alternating.  One JSON line
per record is appended to profiles/blend_bench.jsonl.

    python tools/blend_bench.py [--windows 5] [--launches 200] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "medical-image-editing_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

N, SIDE, CELLS = 4, 512, 16
LEVELS = (3, 5)
SEAM_LEVELS = (1, 2, 3, 4, 5)


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def per_launch_us(sides, windows, launches):
    """{name: fn} -> {name: (median us per launch, [us per window])}: the sides alternate window by window."""
    def loop(fn):
        for _ in range(launches):
            fn()
    for fn in sides.values():
        timed(lambda: loop(fn))
    per = {k: [] for k in sides}
    for _ in range(windows):
        for k, fn in sides.items():
            per[k].append(timed(lambda: loop(fn))[0] / launches * 1e3)
    return {k: (statistics.median(v), [round(t, 2) for t in v]) for k, v in per.items()}


# ------------------------------------------------------------------------------------------------ the plain-torch restatement
def _kernel5(device):
    import torch
    w = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], device=device) / 16.0
    return (w[:, None] * w[None, :]).reshape(1, 1, 5, 5)


def torch_reduce(x, k5):
    import torch.nn.functional as F
    B, C, H, W = x.shape
    return F.conv2d(F.pad(x.reshape(B * C, 1, H, W), (2, 2, 2, 2), mode="replicate"), k5, stride=2).reshape(B, C, H // 2, W // 2)


def torch_expand(x):
    import torch
    import torch.nn.functional as F
    B, C, H, W = x.shape
    p = F.pad(x, (1, 1, 0, 0), mode="replicate")
    a, b, c = p[..., :-2], p[..., 1:-1], p[..., 2:]
    x = torch.stack(((a + 6.0 * b + c) * 0.125, (b + c) * 0.5), dim=4).reshape(B, C, H, 2 * W)
    p = F.pad(x, (0, 0, 1, 1), mode="replicate")
    a, b, c = p[..., :-2, :], p[..., 1:-1, :], p[..., 2:, :]
    return torch.stack(((a + 6.0 * b + c) * 0.125, (b + c) * 0.5), dim=3).reshape(B, C, 2 * H, 2 * W)


def torch_blend(image, edit, cellmask, levels, recon, k5):
    B, C, H, W = image.shape
    h, w = cellmask.shape[1:]
    G = [edit - (image if recon is None else recon)]
    M = [(cellmask != 0).float().repeat_interleave(H // h, 1).repeat_interleave(W // w, 2).reshape(B, 1, H, W)]
    for _ in range(levels):
        G.append(torch_reduce(G[-1], k5))
        M.append(torch_reduce(M[-1], k5))
    R = M[levels] * G[levels]
    for l in range(levels - 1, -1, -1):
        R = M[l] * (G[l] - torch_expand(G[l + 1])) + torch_expand(R)
    return image + R


# ------------------------------------------------------------------------------------------------ the seams
def seam_records(dev):
    import torch
    from dataio.synthetic import synthetic_slice
    import blend_ref as R
    image = torch.stack([synthetic_slice(0, i, SIDE) for i in range(N)]).double()
    mask = torch.zeros(N, CELLS, CELLS, dtype=torch.uint8)
    mask[:, CELLS // 4:3 * CELLS // 4, CELLS // 4:3 * CELLS // 4] = 1
    inside = R.mask_pixels(mask, SIDE, SIDE, torch.float64)
    recon = R.expand(R.reduce(image)) + 0.05
    yy, xx = torch.meshgrid(torch.arange(SIDE, dtype=torch.float64), torch.arange(SIDE, dtype=torch.float64), indexing="ij")
    rr = ((yy - SIDE / 2) ** 2 + (xx - SIDE / 2) ** 2).sqrt()
    bump = 0.5 * ((SIDE * 3 / 16 + 8 - rr) / 16).clamp(0, 1)          # a disc of radius 96 + 8 px with a 16 px edge: 24 px inside the box
    records = []
    for name, edit in (("same_codes", recon), ("lesion", recon + bump)):
        jumps = lambda out: [round(R.boundary_jump(out, mask), 5), round(R.boundary_jump(out - image, mask), 5)]  # noqa: E731
        rec = dict(tool="blend_bench", what="seams", scenario=name, device=dev, shape=[N, SIDE, SIDE, 1], cells=CELLS,
                   region="the central 8 x 8 cells",
                   pictures="synthetic slices; recon = EXPAND(REDUCE(slice)) + 0.05 (a blur and a bias for the first stage's error); edit = "
                            + ("recon: the prior redrew the codes the slice had" if name == "same_codes" else
                               "recon + a smooth disc of height 0.5 that ends 24 px inside the region"),
                   figure="[of the composite, of composite - slice]: the largest |difference| of neighbouring pixels across the region's "
                          "boundary, float64 restatement",
                   slice_itself=round(R.boundary_jump(image, mask), 5), paste=jumps(image * (1 - inside) + edit * inside))
        for source, rc in (("edit", None), ("delta", recon)):
            rec["blend_" + source] = {str(L): jumps(R.blend_ref(image, edit, mask, L, rc)) for L in SEAM_LEVELS}
        records.append(rec)
    return records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blend_bench.jsonl"))
    args = ap.parse_args()

    import torch
    from hipops import ops
    assert torch.cuda.is_available(), "blend_bench measures on the GPU: there is no CPU route"
    dev = torch.cuda.get_device_name(0)
    g = torch.Generator().manual_seed(1)
    image, edit, recon = (torch.randn(N, 1, SIDE, SIDE, generator=g).cuda().contiguous(memory_format=torch.channels_last) for _ in range(3))
    mask = torch.zeros(N, CELLS, CELLS, dtype=torch.uint8)
    mask[:, CELLS // 4:3 * CELLS // 4, CELLS // 4:3 * CELLS // 4] = 1
    mask = mask.cuda()
    k5 = _kernel5("cuda")
    records = []
    picture_bytes = image.numel() * 4
    for levels in LEVELS:
        ws_bytes = 4 * int(ops._L().vqw_blend_cells_workspace(N, SIDE, SIDE, 1, levels))
        for source, rc in (("edit", None), ("delta", recon)):
            ours = lambda: ops.blend_cells(image, edit, mask, levels, rc)  # noqa: E731
            plain = lambda: torch_blend(image, edit, mask, levels, rc, k5)  # noqa: E731
            paste = lambda: ops.paste_cells(image, edit, mask)  # noqa: E731
            err = float((ours() - plain()).abs().max())
            assert err < 1e-4, err
            t = per_launch_us({"ours": ours, "torch": plain, "paste": paste}, args.windows, args.launches)
            floor_bytes = (2 * (2 if rc is None else 3) + 1) * picture_bytes + 2 * ws_bytes
            records.append(dict(tool="blend_bench", what="blend_cells", device=dev, shape=[N, SIDE, SIDE, 1], cells=CELLS, levels=levels,
                                source=source, launches_per_call=2 * levels, workspace_bytes=ws_bytes, floor_bytes=floor_bytes,
                                floor_us_at_5_8_tb_per_s=round(floor_bytes / 5.8e6, 2), ours_us=round(t["ours"][0], 2),
                                torch_us=round(t["torch"][0], 2), paste_us=round(t["paste"][0], 2),
                                speedup_over_torch=round(t["torch"][0] / t["ours"][0], 2), max_abs_diff_from_torch=err,
                                ours_us_windows=t["ours"][1], torch_us_windows=t["torch"][1], paste_us_windows=t["paste"][1]))
    records += seam_records(dev)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for rec in records:
            line = json.dumps(rec)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
