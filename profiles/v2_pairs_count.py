#!/usr/bin/env python3
"""Group iterations of the V pass of scale 0 on the bench's lists, single and paired: a count, from the candidates' maps.

usage: v2_pairs_count.py OUT.json [--calls N]

The bench's context (256x256 synthetic image, 8 x 15, RGB) after its setup, and the first N scheduled slots with the lists the
bench scores on them (seed 1, 4,096 candidates).  Per list: every candidate's palette_map (remap_candidates_device), from it the
pixels the candidate wins (its own index in the tiles of the slot's subpalette), the changed 4-row groups and each group's first
column block (leftmost won column less the filter's reach of four), and per 64-column wave the first group it owns (gs) — the
rule of sparse_v2_body.  A wave with an own group sweeps H/4 + 1 - gs group iterations.  Candidates are paired as the kernel
pairs them: neighbours in the order of first changed group (k_sparse_order; ties in list order here), a repeated colour has no
groups.  Reported per channel class: iterations of the single form, and of the paired form split into wave iterations that
serve two candidates (both resume from min(gsA, gsB)) and one; `extra` = candidate iterations the early start adds.
Load instructions per iteration (sparse_v2_body / sparse_v2_sweep): 5 per candidate without an SSIM map (H plane, a1, r1 twice,
XYB), 9 with one, 7 for a paired wave iteration.  The waves' prologues (checkpoint record, ring priming) are not counted.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import snesimage_amd as S  # noqa: E402
from snesimage_amd.synth import synth_image  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--calls", type=int, default=6)
ap.add_argument("--batch", type=int, default=4096)
args = ap.parse_args()

dev = torch.device("cuda", 0)
image = S.OptimizedImage(synth_image(), 8, 15, device=0)
image.initialize_tiles()
image.recalculate_palettes()
image.optimize()
tiles = torch.from_numpy(image.tile_palettes.reshape(32, 32).astype(np.int64)).to(dev).repeat_interleave(8, 0).repeat_interleave(8, 1)
H4, n = 64, args.batch
d_maps = torch.empty((n, 256, 256), dtype=torch.uint8, device=dev)
tot = {"single_free": 0, "single_ssim": 0, "pair_two": 0, "pair_one": 0, "extra": 0, "live_waves_single": 0, "live_waves_paired": 0}
for i, (method, p, idx, ch, _) in enumerate(S.schedule(8, 15, args.calls)):
    cand = S.random_candidates(1, i, n)
    d_cand = torch.from_numpy(cand).to(dev)
    torch.cuda.synchronize()
    image.remap_candidates_device(p, idx, d_cand.data_ptr(), n, d_maps.data_ptr())
    torch.cuda.synchronize()
    won = (d_maps == idx) & (tiles == p)[None]                                  # [n, 256, 256]
    grp = won.view(n, H4, 4, 256).any(2)                                        # [n, group, x]
    changed = grp.any(2)
    x0 = torch.argmax(grp.to(torch.uint8), 2)                                   # leftmost won column of the group
    gcb = torch.clamp(torch.clamp(x0 - 4, min=0) >> 6, max=3)
    _, first_idx = np.unique(cand, axis=0, return_index=True)                   # a repeated colour: the first holds the items
    holder = torch.zeros(n, dtype=torch.bool, device=dev)
    holder[torch.from_numpy(first_idx).to(dev)] = True
    live = changed[:, :, None] & (gcb[:, :, None] <= torch.arange(4, device=dev)[None, None, :]) & holder[:, None, None]   # [n, g, wave]
    g_ar = torch.arange(H4, device=dev)[None, :, None]
    gs = torch.where(live, g_ar, torch.full_like(g_ar, H4 + 1)).amin(1)         # [n, wave]
    it = torch.clamp(H4 + 1 - gs, min=0)                                        # iterations of the single form
    first = torch.where(changed & holder[:, None], g_ar[:, :, 0], torch.full_like(g_ar[:, :, 0], H4)).amin(1)
    order = torch.argsort(first, stable=True)
    a, b = gs[order[0::2]], gs[order[1::2]]
    both = (a <= H4) & (b <= H4)
    two = torch.where(both, H4 + 1 - torch.minimum(a, b), torch.zeros_like(a)).sum().item()
    one = torch.where(~both, torch.clamp(H4 + 1 - torch.minimum(a, b), min=0), torch.zeros_like(a)).sum().item()
    single = it.sum().item()
    tot["single_free"] += single
    tot["single_ssim"] += single
    tot["pair_two"] += two
    tot["pair_one"] += one
    tot["extra"] += 2 * two + one - single
    tot["live_waves_single"] += int((gs <= H4).sum().item())
    tot["live_waves_paired"] += int(both.sum().item() + ((a <= H4) ^ (b <= H4)).sum().item())
k = float(args.calls)
per = {key: v / k for key, v in tot.items()}
res = {"what": "group iterations of one channel of scale 0 per 4,096-candidate call, mean of the first %d scheduled calls of the bench's run" % args.calls,
       "per_channel": per,
       "paired_share_of_candidate_iterations": 2 * per["pair_two"] / (2 * per["pair_two"] + per["pair_one"]),
       "extra_share_of_single_iterations": per["extra"] / per["single_free"],
       "loads_per_launch_steady_state": {
           "single_6_scales": per["single_free"] * (5 + 5 + 9),
           "paired_6_scales": 2 * (7 * per["pair_two"] + 5 * per["pair_one"]) + 9 * per["single_ssim"]}}
json.dump(res, open(args.out, "w"), indent=1)
print(json.dumps(res))
