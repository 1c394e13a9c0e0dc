"""What the shared backdrop colour (SNES_BACKDROP) costs and what it buys, 256 x 256, one MI355X.

    python profiles/backdrop.py [--repeats R] [--baseline DIR] [--out profiles/backdrop.json]

1. Tied call: one 64-candidate call on the backdrop slot of an (8,15) + backdrop context (dense path, pack mode 3) against a
   regular 64-candidate call of a plain (8,16) context with SNES_SPARSE=0 (the same dense stages) — RGB, perceptual, dither.
2. Sweep: snesimage_run_slots calls per second, (8,15) + backdrop against plain (8,16) — RGB and dither.
3. Gain: error after 2,400 calls from the k-means start for plain (C,S), (C,S) + backdrop and plain (C,S+1), (8,15) and
   (8,3), four synthetic seeds, RGB and dither.

--baseline DIR: a checkout of the commit to compare with (its library built): the plain legs of 1 and 2 run from it; without
it they run from this tree.  Every measurement is a child process of its own under a time limit; the legs of a comparison
alternate (A B A B ...), and every figure is the mean of its repeats with their lowest and highest value beside it.  A child
that fails ends the run: nothing more is started on the device."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = {"rgb": {}, "perceptual": {"perceptual": True}, "dither": {"dither": True}}


def make(S, img, count, size, flags, backdrop):
    g = S.OptimizedImage(img, count, size, backdrop=True, **flags) if backdrop else S.OptimizedImage(img, count, size, **flags)
    g.initialize_tiles()
    g.recalculate_palettes()
    return g


def child(a):
    sys.path.insert(0, a.root)
    import snesimage_amd as S
    from snesimage_amd.synth import synth_image
    flags = FLAGS[a.flags]
    if a.child == "call":  # ms per 64-candidate call on one slot, host clock around synchronous steps
        g = make(S, synth_image(0x5EED0000), 8, 15 if a.backdrop else 16, flags, a.backdrop)
        p, i = (8, 0) if a.backdrop else (0, 15)
        for j in range(6):
            g.step(S.METHOD_RANDOM, p, i, 0, 1, j)
        t0 = time.perf_counter()
        for j in range(6, 6 + a.n):
            g.step(S.METHOD_RANDOM, p, i, 0, 1, j)
        print(json.dumps({"ms_per_call": 1e3 * (time.perf_counter() - t0) / a.n}))
    elif a.child == "sweep":  # calls per second of the reference's loop through the slot windows
        g = make(S, synth_image(0x5EED0000), 8, 15 if a.backdrop else 16, flags, a.backdrop)
        _, st, _ = g.run_slots(a.n // 4, seed=1, first_step_id=0, want_log=False)
        g.sync()
        t0 = time.perf_counter()
        _, st, stats = g.run_slots(a.n, seed=1, first_step_id=a.n // 4, state=st, want_log=False)
        g.sync()
        print(json.dumps({"calls_per_s": a.n / (time.perf_counter() - t0), "accepted": stats["accepted"]}))
    else:  # gain: error after a.n calls
        out = {}
        for size in (15, 3):
            for seed in range(4):
                img = synth_image(0x5EED0000 + seed)
                for name, sz, bd in (("plain", size, False), ("backdrop", size, True), ("plus_one", size + 1, False)):
                    g = make(S, img, 8, sz, flags, bd)
                    e0 = g.error()
                    g.run_slots(a.n, seed=1, want_log=False)
                    out["%d/%s/%d" % (size, name, seed)] = {"start": e0, "end": g.error()}
                    g.close()
        print(json.dumps(out))
    return 0


def run_child(a, root, kind, flags, backdrop, n, env=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--flags", flags, "--n", str(n), "--root", root] + (["--backdrop"] if backdrop else [])
    r = subprocess.run(cmd, env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=a.timeout * (3 if kind == "gain" else 1))
    if r.returncode != 0:
        print(json.dumps({"failed": cmd[2:], "rc": r.returncode, "stderr": r.stderr[-600:]}), flush=True)
        sys.exit(1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def stat(v):
    return {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backdrop.json"))
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--skip-gain", action="store_true")
    ap.add_argument("--child", choices=["call", "sweep", "gain"])
    ap.add_argument("--flags", default="rgb")
    ap.add_argument("--backdrop", action="store_true")
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    base = os.path.abspath(a.baseline) if a.baseline else ROOT
    res = {"baseline": "another checkout" if a.baseline else "this tree", "call_ms": {}, "sweep_calls_per_s": {}, "gain": {}}
    for fl in ("rgb", "perceptual", "dither"):
        tied, plain = [], []
        for _ in range(a.repeats):  # alternating
            tied.append(run_child(a, ROOT, "call", fl, True, 40)["ms_per_call"])
            plain.append(run_child(a, base, "call", fl, False, 40, {"SNES_SPARSE": "0"})["ms_per_call"])
        res["call_ms"][fl] = {"tied_8x15_backdrop": stat(tied), "dense_regular_8x16": stat(plain)}
        print(json.dumps({"call_ms": fl, **res["call_ms"][fl]}), flush=True)
    for fl in ("rgb", "dither"):
        bd, plain = [], []
        n = 1452 if fl == "rgb" else 484  # whole sweeps of the (8,15) + backdrop schedule (121 calls each)
        for _ in range(a.repeats):
            bd.append(run_child(a, ROOT, "sweep", fl, True, n)["calls_per_s"])
            plain.append(run_child(a, base, "sweep", fl, False, n)["calls_per_s"])
        res["sweep_calls_per_s"][fl] = {"8x15_backdrop": stat(bd), "plain_8x16": stat(plain)}
        print(json.dumps({"sweep": fl, **res["sweep_calls_per_s"][fl]}), flush=True)
    if not a.skip_gain:
        for fl in ("rgb", "dither"):
            res["gain"][fl] = run_child(a, ROOT, "gain", fl, False, 2400)
            print(json.dumps({"gain": fl, **res["gain"][fl]}), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
