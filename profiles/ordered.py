"""What ordered dithering (snesimage_set_ordered_dither) costs beside no dithering and beside --dither: the bench image
(256 x 256, 8 x 15, RGB), one MI355X.

    python profiles/ordered.py [--calls 4000] [--repeats R] [--baseline DIR] [--out profiles/ordered_rgb.json]

Legs: no table, Bayer 4 x 4 and 8 x 8 at amplitude 32, and --dither (Floyd-Steinberg).  Every leg starts from the k-means
initialisers, runs `--calls` calls of the reference's loop through snesimage_run_slots (64 candidates per random call) and
then reports
  ms_per_4096    one 4,096-candidate call (snesimage_step, host clock around synchronous calls, slots in schedule order);
  calls_per_s    snesimage_run_slots over the 960 calls that follow a 120-call warm-up, continuing its scheduler state;
  contested      pixels per slot whose map names the slot's entry for at least one of a call's 64 random candidates, mean over
                 the 120 slots (from the maps of snesimage_remap_candidates_device).  This counts the pixels the incumbent
                 colour already held as well, so it is an upper bound on what the group-sparse scorer's contested list
                 (k_build_plist) holds, not that list's length;
  groups         4-row groups of scale 0 (H / 4 = 64 of them) in which a candidate wins a pixel, mean over those candidates:
                 what the group-sparse scorer has to recompute per candidate;
  error          error() after the `--calls` calls (every leg ran the same number).
--baseline DIR: a checkout of the parent commit (its library built): the no-table and --dither legs also run from it, the
legs alternating.  Every measurement is a child process of its own under a time limit; a child that fails ends the run:
nothing more is started on the device.  The output is stamped with the library's source hash."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {"none": (None, False), "ordered4": (4, False), "ordered8": (8, False), "dither": (None, True)}


def child(a):
    sys.path.insert(0, a.root)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import snesimage_amd as S
    from snesimage_amd import _ffi
    from snesimage_amd.synth import synth_image
    n, dither = LEGS[a.leg]
    g = S.OptimizedImage(synth_image(0x5EED0000), 8, 15, dither=dither)
    if n:
        g.set_ordered_dither(S.bayer_offsets(n, a.amplitude))
    g.initialize_tiles()
    g.recalculate_palettes()
    e0 = g.error()
    _, st, stats = g.run_slots(a.calls, seed=1, first_step_id=0, want_log=False)
    out = {"leg": a.leg, "version": _ffi.load().snesimage_version().decode(), "error_start": e0, "error": g.error(), "calls": a.calls,
           "accepted": stats["accepted"]}
    _, st, _ = g.run_slots(120, seed=1, first_step_id=a.calls, state=st, want_log=False)  # warm-up of the timed window
    g.sync()
    t0 = time.perf_counter()
    _, st, stats = g.run_slots(960, seed=1, first_step_id=a.calls + 120, state=st, want_log=False)  # the loop's next 960 calls
    g.sync()
    out["calls_per_s"] = 960 / (time.perf_counter() - t0)
    out["accepted_timed"] = stats["accepted"]
    if not dither:  # what a call of 64 random candidates contests, slot by slot (the state is left as it is)
        from hipmem import DeviceArray
        d_m = DeviceArray((64, 256, 256), np.uint8, fill=0)
        contested, groups = [], []
        for p in range(8):
            for i in range(15):
                d_c = DeviceArray.from_numpy(S.random_candidates(2, p * 15 + i, 64))
                g.remap_candidates_device(p, i, d_c.ptr, 64, d_m.ptr)
                g.sync()
                won = (d_m.numpy() == i) & (g.tile_palettes.reshape(32, 32).repeat(8, 0).repeat(8, 1) == p)[None]
                contested.append(int(won.any(0).sum()))
                per = won.reshape(64, 64, 4 * 256).any(2).sum(1)
                groups += [int(v) for v in per if v]
                d_c.free()
        out["contested"] = sum(contested) / len(contested)
        out["groups"] = sum(groups) / max(1, len(groups))
    sched = S.schedule(8, 15, 40)
    for j, (_, p, i, _, _) in enumerate(sched[:8]):
        g.step(S.METHOD_RANDOM, p, i, 0, 3, j, 4096)
    t0 = time.perf_counter()
    for j, (_, p, i, _, _) in enumerate(sched[8:8 + a.steps]):
        g.step(S.METHOD_RANDOM, p, i, 0, 3, 8 + j, 4096)
    out["ms_per_4096"] = 1e3 * (time.perf_counter() - t0) / a.steps
    print(json.dumps(out))
    return 0


def run_child(a, root, leg):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--leg", leg, "--root", root, "--calls", str(a.calls), "--steps", str(a.steps),
           "--amplitude", str(a.amplitude)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        print(json.dumps({"failed": cmd[2:], "rc": r.returncode, "stderr": r.stderr[-600:]}), flush=True)
        sys.exit(1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--amplitude", type=int, default=32)
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ordered_rgb.json"))
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--leg", choices=sorted(LEGS), default="none")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"runs": []}
    for _ in range(a.repeats):  # the legs alternate
        for leg in ("none", "ordered4", "ordered8", "dither"):
            r = run_child(a, ROOT, leg)
            res["runs"].append(r)
            print(json.dumps(r), flush=True)
            if a.baseline and leg in ("none", "dither"):
                r = run_child(a, os.path.abspath(a.baseline), leg)
                r["leg"] = "parent_" + leg
                res["runs"].append(r)
                print(json.dumps(r), flush=True)
    res["library"] = next(r["version"] for r in res["runs"] if not r["leg"].startswith("parent_"))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
