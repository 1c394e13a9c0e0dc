"""What the backdrop colour of a shared-palette set costs and buys (DESIGN §5c''): F frames of 256 x 224, 8 subpalettes x 15
colours, RGB, 64 candidates per random call, F in {2, 4, 8}.  One JSON line per measurement; every measurement runs in a
child process of its own under a time limit, and a failed child ends the run.

    python profiles/set_backdrop.py [--frames 2,4,8] [--what call,slots] [--out profiles/set_backdrop.json]

call:  ms per optimizer call, host clock around snesimage_shared_step (which ends in a synchronising read of the record), the
       three legs alternating, REPEATS rounds of CALLS calls each behind a warm-up round: a backdrop call of the set (the
       members' dense tied paths on their own streams + ks_commit_tied), a regular call of the same set (the batched
       group-sparse launches + ks_commit), and a backdrop call of ONE backdrop context (snesimage_step), to be read times F.
slots: calls per second of run_slots(window=0) over TIMED calls behind a run-in of RUN_IN calls, on the backdrop set and on the
       plain set of the same frames, and E of each after the same RUN_IN + TIMED calls (what B buys at an equal number of
       calls; a backdrop sweep has 121 slots, a plain one 120).
Frame i is synth_image(0x5EED0000 + i, 256, 224), as in profiles/shared_slots.py."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS, REPEATS = 20, 5
TIMED, RUN_IN = 484, 968  # whole backdrop sweeps: 4 and 8 of them


def make(S, F, backdrop):
    from snesimage_amd.synth import synth_image
    imgs = [S.OptimizedImage(synth_image(0x5EED0000 + i, 256, 224), 8, 15, backdrop=backdrop) for i in range(F)]
    for g in imgs:
        g.set_chunk(64)
    sp = S.SharedPalette(imgs, backdrop=True if backdrop else None)
    sp.initialize_tiles()
    sp.recalculate_palettes()
    return imgs, sp


def child_call(F):
    sys.path.insert(0, ROOT)
    import snesimage_amd as S
    from snesimage_amd import _ffi
    from snesimage_amd.synth import synth_image
    imgs, sp = make(S, F, True)
    one = S.OptimizedImage(synth_image(0x5EED0000, 256, 224), 8, 15, backdrop=True)
    one.set_chunk(64)
    one.initialize_tiles()
    one.recalculate_palettes()
    legs = {"set_backdrop_call": lambda j: sp.step(S.METHOD_RANDOM, 8, 0, 0, 1, j), "set_regular_call": lambda j: sp.step(S.METHOD_RANDOM, j % 8, j % 15, 0, 1, j),
            "single_backdrop_call": lambda j: one.step(S.METHOD_RANDOM, 8, 0, 0, 1, j)}
    ms = {k: [] for k in legs}
    step_id = 0
    for rnd in range(REPEATS + 1):  # round 0 warms every leg up (workspaces, code objects)
        for name, leg in legs.items():
            t0 = time.perf_counter()
            for _ in range(CALLS):
                leg(step_id)
                step_id += 1
            if rnd:
                ms[name].append((time.perf_counter() - t0) * 1e3 / CALLS)
    out = {"what": "call", "frames": F, "calls_per_round": CALLS, "rounds": REPEATS, "build": _ffi.load().snesimage_version().decode()}
    for name, v in ms.items():
        out[name + "_ms"] = {"mean": round(sum(v) / len(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out["F_times_single_ms"] = round(F * out["single_backdrop_call_ms"]["mean"], 4)
    sp.close()
    for g in imgs + [one]:
        g.close()
    print(json.dumps(out))


def child_slots(F, backdrop):
    sys.path.insert(0, ROOT)
    import snesimage_amd as S
    from snesimage_amd import _ffi
    imgs, sp = make(S, F, backdrop)
    e0 = sp.error()
    _, st, _ = sp.run_slots(RUN_IN, seed=1, want_log=False)
    t0 = time.perf_counter()
    log, st, stats = sp.run_slots(TIMED, seed=1, first_step_id=RUN_IN, state=st, window=0)
    dt = time.perf_counter() - t0
    out = {"what": "slots", "frames": F, "backdrop": bool(backdrop), "calls": TIMED, "run_in": RUN_IN, "calls_per_s": round(TIMED / dt, 1),
           "acceptance": round(stats["accepted"] / TIMED, 4), "launch_sets": stats["windows"], "error_start": e0, "error": log[-1][0],
           "build": _ffi.load().snesimage_version().decode()}
    if backdrop:
        out["backdrop_rgb5"] = sp.backdrop.tolist()
    sp.close()
    for g in imgs:
        g.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="2,4,8")
    ap.add_argument("--what", default="call,slots")
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=3, metavar=("WHAT", "F", "BACKDROP"))
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "call":
            child_call(int(a.child[1]))
        else:
            child_slots(int(a.child[1]), a.child[2] == "1")
        return 0
    lines = []
    for F in [int(v) for v in a.frames.split(",")]:
        jobs = ([("call", "1")] if "call" in a.what.split(",") else []) + ([("slots", "1"), ("slots", "0")] if "slots" in a.what.split(",") else [])
        for what, bd in jobs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", what, str(F), bd]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print(json.dumps({"what": what, "frames": F, "error": "timeout"}))
                return 1
            if r.returncode != 0:
                print(json.dumps({"what": what, "frames": F, "rc": r.returncode, "stderr": r.stderr[-400:]}))
                return 1  # a failed child ends the run: nothing more is started on the device
            line = r.stdout.strip().splitlines()[-1]
            lines.append(json.loads(line))
            print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
