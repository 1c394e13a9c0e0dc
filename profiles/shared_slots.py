"""Calls per second of the reference's loop on one palette shared by F frames of 256 x 224 (a set): slot
windows (snesimage_shared_run_slots, window = 0) against call by call.  RGB, 8 subpalettes x 15 colours, 64 candidates per
random call, F in {1, 2, 4, 8}, in two states: the first 480 calls from the k-means initialisers ("start"), and 480 calls
after a run-in of 4,000 calls ("run-in").  One JSON line per (F, state, mode); every measurement runs in a child process
of its own under a time limit, and a failed child ends the run.

    python profiles/shared_slots.py [--frames 1,2,4,8] [--modes window0,window1,loop] [--states start,run-in]

Modes: window0 = run_slots(window=0); window1 = run_slots(window=1), the library's own call-by-call path; loop =
SharedPalette.run, the Python loop of snesimage_shared_step_async + snesimage_shared_last_step (the one mode a build
without the windows has: run this file against the parent commit for the yardstick).  Frame i is
synth_image(0x5EED0000 + i, 256, 224), as in profiles/shared.py.  All modes walk the same trajectory (bit-identical), so
the acceptance rate of a line belongs to its state, not to its mode."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMED, RUN_IN = 480, 4000


def child(F, state, mode):
    sys.path.insert(0, ROOT)
    import snesimage_amd as S
    from snesimage_amd import _ffi
    from snesimage_amd.synth import synth_image
    imgs = [S.OptimizedImage(synth_image(0x5EED0000 + i, 256, 224), 8, 15) for i in range(F)]
    for g in imgs:
        g.set_chunk(64)
    sp = S.SharedPalette(imgs)
    sp.initialize_tiles()
    sp.recalculate_palettes()
    have = hasattr(sp, "run_slots")
    st, first = (0, 0, 0, 0), 0
    if state == "run-in":
        if have:
            _, st, _ = sp.run_slots(RUN_IN, seed=1, want_log=False)
        else:
            _, st = sp.run(RUN_IN, seed=1)
        first = RUN_IN
    elif have and mode == "window0":
        sp.reserve_slots(64)  # the slot contexts' allocation is not what is timed
    t0 = time.perf_counter()
    if mode == "loop":
        log, st = sp.run(TIMED, seed=1, first_step_id=first, state=st)
        stats = {"windows": TIMED, "scored": 0, "useful": 0, "accepted": sum(1 for _, k, _, _ in log if k >= 0)}
    else:
        log, st, stats = sp.run_slots(TIMED, seed=1, first_step_id=first, state=st, window=0 if mode == "window0" else 1)
    dt = time.perf_counter() - t0
    out = {"frames": F, "state": state, "mode": mode, "calls": TIMED, "calls_per_s": round(TIMED / dt, 1),
           "acceptance": round(stats["accepted"] / TIMED, 4), "launch_sets": stats["windows"],
           "useful_share": round(stats["useful"] / stats["scored"], 4) if stats["scored"] else None,
           "error": log[-1][0], "build": _ffi.load().snesimage_version().decode()}
    sp.close()
    for g in imgs:
        g.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,2,4,8")
    ap.add_argument("--modes", default="window0,window1,loop")
    ap.add_argument("--states", default="start,run-in")
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", nargs=3, metavar=("F", "STATE", "MODE"))
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), a.child[1], a.child[2])
        return 0
    for F in [int(v) for v in a.frames.split(",")]:
        for state in a.states.split(","):
            for mode in a.modes.split(","):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", str(F), state, mode]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
                except subprocess.TimeoutExpired:
                    print(json.dumps({"frames": F, "state": state, "mode": mode, "error": "timeout"}))
                    return 1
                if r.returncode != 0:
                    print(json.dumps({"frames": F, "state": state, "mode": mode, "rc": r.returncode, "stderr": r.stderr[-400:]}))
                    return 1  # a failed child ends the run: nothing more is started on the device
                print(r.stdout.strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
