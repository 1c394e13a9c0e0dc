"""ms per optimizer call for one palette shared by F frames of 256 x 224 (a set) against F separate
single-image calls (one snesimage_step per frame).  RGB, 8 subpalettes x 15 colours, random candidates; F in {1, 2, 4, 8}
at 64 candidates per call and F in {1, 2, 4} at 4,096 (each member's storage is ~4.45 MB per candidate: 18 GB at 4,096).
One JSON line per (F, candidates, mode); every measurement runs in a child process of its own under a time limit.

    python profiles/shared.py [--steps K] [--warmup W]

Frame i is synth_image(0x5EED0000 + i, 256, 224).  Both modes start from the same kind of state: the shared leg from the
set's initialisers, the separate leg from every frame's own.  Calls walk the slots as the reference's scheduler does and
every call waits for its result (snesimage_shared_step / snesimage_step)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(F, n, shared, steps, warmup):
    sys.path.insert(0, ROOT)
    import snesimage_amd as S
    from snesimage_amd.synth import synth_image
    imgs = [S.OptimizedImage(synth_image(0x5EED0000 + i, 256, 224), 8, 15) for i in range(F)]
    for g in imgs:
        g.set_chunk(n)
    slots = [(p, i) for p in range(8) for i in range(15)]
    if shared:
        sp = S.SharedPalette(imgs)
        sp.initialize_tiles()
        sp.recalculate_palettes()

        def call(j):
            p, i = slots[j % len(slots)]
            return sp.step(S.METHOD_RANDOM, p, i, 0, 1, j, n)[0]
    else:
        for g in imgs:
            g.initialize_tiles()
            g.recalculate_palettes()

        def call(j):
            p, i = slots[j % len(slots)]
            return sum(g.step(S.METHOD_RANDOM, p, i, 0, 1, j, n)[0] for g in imgs)
    for j in range(warmup):
        call(j)
    t0 = time.perf_counter()
    for j in range(warmup, warmup + steps):
        err = call(j)
    dt = time.perf_counter() - t0
    if shared:
        sp.close()
    for g in imgs:
        g.close()
    print(json.dumps({"frames": F, "candidates_per_call": n, "mode": "shared" if shared else "separate", "steps": steps,
                      "ms_per_call": round(1e3 * dt / steps, 4), "error": err}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", nargs=3, type=int, metavar=("F", "N", "SHARED"))
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], bool(a.child[2]), a.steps, a.warmup)
        return 0
    cases = [(F, 64) for F in (1, 2, 4, 8)] + [(F, 4096) for F in (1, 2, 4)]
    for F, n in cases:
        for shared in (1, 0):
            cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup), "--child", str(F), str(n), str(shared)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print(json.dumps({"frames": F, "candidates_per_call": n, "shared": shared, "error": "timeout"}))
                return 1
            if r.returncode != 0:
                print(json.dumps({"frames": F, "candidates_per_call": n, "shared": shared, "rc": r.returncode, "stderr": r.stderr[-400:]}))
                return 1  # a failed child ends the run: nothing more is started on the device
            print(r.stdout.strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
