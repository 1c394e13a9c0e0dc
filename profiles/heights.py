"""Candidates per second and ms per optimizer call at 256, 240 and 224 rows (RGB, 8 subpalettes x 15 colours), once on the
group-sparse path and once on the dense path (SNES_SPARSE=0).  One JSON line per (height, path); every measurement runs in
a child process of its own under a time limit.

    python profiles/heights.py [--steps K] [--warmup W] [--heights 256,240,224]

The sparse leg scores 4,096 random candidates per call; the dense leg 1,024 (its workspace is ~3.5 MB per candidate).
Every height crops the same 256-row synthetic picture (seed 0x5EED0000, bench.py's) to its top rows, so that the lines differ
in the height alone.  Calls walk the slots as the reference's scheduler does (palette, then index) and commit as step() does."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(h, sparse, n, steps, warmup):
    sys.path.insert(0, ROOT)
    import numpy as np

    import snesimage_amd as S
    from snesimage_amd.synth import synth_image
    img = np.ascontiguousarray(synth_image(0x5EED0000, 256, 256)[:h])  # the top h rows of one picture: only the height differs
    g = S.OptimizedImage(img, 8, 15)
    g.set_chunk(n)
    g.initialize_tiles()
    g.recalculate_palettes()
    slots = [(p, i) for p in range(8) for i in range(15)]
    for j in range(warmup):
        p, i = slots[j % len(slots)]
        g.step(S.METHOD_RANDOM, p, i, 0, 1, j, n)
    t0 = time.perf_counter()
    for j in range(warmup, warmup + steps):
        p, i = slots[j % len(slots)]
        err, _ = g.step(S.METHOD_RANDOM, p, i, 0, 1, j, n)
    dt = time.perf_counter() - t0
    g.close()
    print(json.dumps({"height": h, "path": "sparse" if sparse else "dense", "candidates_per_call": n, "steps": steps,
                      "ms_per_step": round(1e3 * dt / steps, 4), "cand_per_s": round(n * steps / dt), "error": err}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--heights", default="256,240,224")
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--child", nargs=3, type=int, metavar=("H", "SPARSE", "N"))
    a = ap.parse_args()
    if a.child:
        h, sparse, n = a.child
        child(h, bool(sparse), n, a.steps, a.warmup)
        return 0
    rc = 0
    for sparse, n in ((1, 4096), (0, 1024)):
        for h in (int(v) for v in a.heights.split(",")):
            env = dict(os.environ, SNES_SPARSE=str(sparse))
            cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup), "--child", str(h), str(sparse), str(n)]
            try:
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print(json.dumps({"height": h, "path": "sparse" if sparse else "dense", "error": "timeout"}))
                return 1
            if r.returncode != 0:
                print(json.dumps({"height": h, "path": "sparse" if sparse else "dense", "rc": r.returncode, "stderr": r.stderr[-400:]}))
                return 1  # a failed child ends the run: nothing more is started on the device
            print(r.stdout.strip().splitlines()[-1], flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
