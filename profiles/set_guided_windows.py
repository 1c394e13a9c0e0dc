"""What the guided calls of a set cost through the set's slot windows (snesimage_shared_guided_run_slots, DESIGN 5f'''') against the
parent commit's snesimage_shared_guided_sweep, and what the windows' generator costs against single generators.  One MI355X.

    python profiles/set_guided_windows.py --parent DIR [--reps 2] [--samples 3] [--k 16] [--out profiles/set_guided_windows.json] [--md FILE]

The legs of BASELINE.md's "Guided calls of a set": frames synth_image(0x5EED5B00 + f, 256, 224), F = 2, 4 and 8, 8 x 15 and 1 x 15,
RGB, K = 16, chunk 64; from the set's k-means start, and after 1,200 calls of the plain schedule through the set's slot windows.
Every leg is a child process of its own under a time limit (a child that fails ends the run: nothing more is started on the
device).  Per configuration the parent's child and this tree's child alternate `--reps` times; inside a child every kind of run
is timed `--samples` times, the kinds in turn, each from the same state (the palette is put back and optimize() run, untimed):
  parent      (--parent DIR: a tree of the parent commit, built) whole snesimage_shared_guided_sweep calls, by the host clock,
              each ending in its own read-back;
  this tree   the same number of calls through snesimage_shared_guided_run_slots at window 0, 1, 8 and 64 (clipped to 64 / F), with
              its stats; and the generator: the window generator for a window of min(64 / F, slots) consecutive slots through
              snesimage_shared_debug_guided_window_costs against as many snesimage_shared_guided_costs — both with their tables read back.
The output is stamped with the library's source hash."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = (0, 1, 8, 64)


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def spread(v):
    return dict(median=pct(v, 0.5), lo=min(v), hi=max(v), n=len(v))


def child(a):
    import numpy as np  # noqa: F401
    import snesimage_amd as S
    from snesimage_amd.synth import synth_image
    ctxs = [S.OptimizedImage(synth_image(0x5EED5B00 + f, 256, 224), a.c, a.s) for f in range(a.frames)]
    for c in ctxs:
        c.set_chunk(64)
    sp = S.SharedPalette(ctxs)
    sp.initialize_tiles()
    sp.recalculate_palettes()
    if a.start == "converged":
        sp.run_slots(1200, seed=1, want_log=False)
    new = hasattr(S.SharedPalette, "guided_run_slots")
    slots = a.c * a.s
    sweeps = 2 if a.c > 1 else 8
    n = sweeps * slots
    pal = sp.palette

    def reset():
        sp.palette = pal
        sp.error()

    out = dict(frames=a.frames, c=a.c, s=a.s, start=a.start, calls=n, new=new, version=S._ffi.load().snesimage_version().decode(), runs={}, stats={})

    def timed(fn):
        t0 = time.perf_counter()
        st = fn()
        sp.error()  # (ends in a device synchronise)
        return time.perf_counter() - t0, st

    def sweep_run():
        for _ in range(sweeps):
            sp.guided_sweep(a.k)

    kinds = [("sweep", sweep_run)]
    if new:
        for w in WINDOWS:
            kinds.append(("window %d" % w, lambda w=w: sp.guided_run_slots(n, a.k, window=w, want_log=False)[2]))
    for name, fn in kinds:  # untimed: the allocations and the first launches
        fn()
        reset()
    for _ in range(a.samples):
        for name, fn in kinds:
            secs, st = timed(fn)
            out["runs"].setdefault(name, []).append(n / secs)
            if st:
                out["stats"][name] = st
            reset()
    if new:
        K = min(64 // a.frames, slots)
        win = [(j // a.s, j % a.s) for j in range(K)]
        sp.debug_guided_window_costs(win)
        for p, i in win:
            sp.guided_costs(p, i)
        gen = dict(calls=K, window_ms=[], singles_ms=[])
        for _ in range(a.samples):
            t0 = time.perf_counter()
            sp.debug_guided_window_costs(win)
            gen["window_ms"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            for p, i in win:
                sp.guided_costs(p, i)
            gen["singles_ms"].append(1e3 * (time.perf_counter() - t0))
        out["generator"] = gen
    print(json.dumps(out))


def run_child(a, root, extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--k", str(a.k), "--samples", str(a.samples)] + [str(x) for x in extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        print(json.dumps({"failed": cmd[2:], "rc": r.returncode, "stderr": r.stderr[-600:]}), flush=True)
        sys.exit(1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def markdown(res):
    f = lambda d: "%.0f (%.0f – %.0f)" % (d["median"], d["lo"], d["hi"])
    names = ["parent sweep", "sweep"] + ["window %d" % w for w in WINDOWS]
    L = ["| frames | geometry | start | " + " | ".join(names) + " | window 0: launch sets, useful / scored | generator, window of K / K singles, ms |", "|---|---|---|" + "---|" * (len(names) + 2)]
    for r in res["legs"]:
        st = r["stats"].get("window 0", {})
        g = r.get("generator")
        L.append("| %d x 256 x 224 | %d x %d | %s | %s | %d, %.3f | %s |" % (
            r["frames"], r["c"], r["s"], r["start"], " | ".join(f(r["calls_per_s"][n]) if n in r["calls_per_s"] else "-" for n in names), st.get("windows", 0),
            st.get("useful", 0) / max(1, st.get("scored", 0)), "K = %d: %.2f / %.2f" % (g["calls"], pct(g["window_ms"], 0.5), pct(g["singles_ms"], 0.5)) if g else "-"))
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--parent", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_guided_windows.json"))
    ap.add_argument("--md", default="")
    ap.add_argument("--timeout", type=int, default=150)
    ap.add_argument("--frames-list", default="2,4,8")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--c", type=int, default=8)
    ap.add_argument("--s", type=int, default=15)
    ap.add_argument("--start", default="kmeans")
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, a.root)
        return child(a)
    res = dict(k=a.k, reps=a.reps, samples=a.samples, legs=[])
    for F in [int(x) for x in a.frames_list.split(",")]:
        for c, s in ((8, 15), (1, 15)):
            for start in ("kmeans", "converged"):
                rates, stats, gen = {}, {}, None
                for rep in range(a.reps):  # alternating
                    roots = ([("parent", os.path.abspath(a.parent))] if a.parent else []) + [("this", ROOT)]
                    for who, root in roots:
                        r = run_child(a, root, ["--frames", F, "--c", c, "--s", s, "--start", start])
                        res["version" if who == "this" else "parent_version"] = r["version"]
                        for name, v in r["runs"].items():
                            rates.setdefault("parent sweep" if who == "parent" else name, []).extend(v)
                        if who == "this":
                            stats = r["stats"]
                            if r.get("generator"):
                                gen = gen or dict(calls=r["generator"]["calls"], window_ms=[], singles_ms=[])
                                gen["window_ms"] += r["generator"]["window_ms"]
                                gen["singles_ms"] += r["generator"]["singles_ms"]
                row = dict(frames=F, c=c, s=s, start=start, calls_per_s={n: spread(v) for n, v in rates.items()}, samples=rates, stats=stats, generator=gen)
                print(json.dumps(dict(frames=F, c=c, s=s, start=start, calls_per_s={n: round(d["median"]) for n, d in row["calls_per_s"].items()}, generator=gen and [pct(gen["window_ms"], 0.5), pct(gen["singles_ms"], 0.5)])), flush=True)
                res["legs"].append(row)
                with open(a.out, "w") as f:  # (kept after every configuration: a run cut short leaves what it measured)
                    json.dump(res, f, indent=1, sort_keys=True)
    md = markdown(res)
    if a.md:
        with open(a.md, "w") as f:
            f.write(md)
    print(md)


if __name__ == "__main__":
    main()
