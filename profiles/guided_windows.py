"""What guided calls through the slot windows (snesimage_guided_run_slots, DESIGN 5f''') do to the rate of guided calls and to the
equal-time comparison that guided calls lost while they were stepped call by call.  One MI355X.

    python profiles/guided_windows.py [--parent DIR] [--reps 5] [--k 16] [--out profiles/guided_windows.json] [--md FILE]

Every leg is a child process of its own under a time limit (a child that fails ends the run: nothing more is started on the
device); the legs of a comparison alternate, `--reps` times.  synth_image() at 8 x 15, RGB, K = 16.
  rate   256 x 256 and 256 x 224; from the k-means start, and after 2,400 calls of the plain loop.  One sample = 10 guided sweeps
         (1,200 calls) by the host clock, ending in a device synchronise, after an untimed warm-up that makes the allocations
         (the state is put back behind it).  This tree: snesimage_guided_run_slots at window 0, 8 and 64 with its stats;
         --parent DIR (a tree of the parent commit, built): ten snesimage_guided_sweep, timed by the same code.
  equal  the plain schedule for 2,400 calls through the slot windows against the schedule with one guided sweep behind every
         sweep of the palette (cli --guided 1), the guided sweeps through the windows as well, run until the plain run's seconds
         have passed: E at 25 / 50 / 100 % of the plain run's wall-clock.  Both in pieces of at most 60 calls, the host clock
         read behind each.  The four pictures of the "Gain" table of profiles/guided.py.
The output is stamped with the library's source hash."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PICTURES = [("bench 256 x 256", None, 256), ("seed 11 256 x 256", 11, 256), ("seed 12 256 x 256", 12, 256), ("bench 256 x 224", None, 224)]
C, SZ, PIECE = 8, 15, 60


def picture(seed, h):
    from snesimage_amd.synth import synth_image
    return synth_image(h=h) if seed is None else synth_image(seed, 256, h)


def started(S, seed, h):
    g = S.OptimizedImage(picture(seed, h), C, SZ)
    g.initialize_tiles()
    g.recalculate_palettes()
    return g


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def spread(v):
    return dict(median=pct(v, 0.5), p10=pct(v, 0.1), p90=pct(v, 0.9), n=len(v))


def warm(g, k, windows):
    """The allocations and the first launches, untimed; the state is put back."""
    pal = g.palette
    g.slots_reserve(64)
    g.run_slots(16, seed=9, want_log=False)
    if windows:
        g.guided_run_slots(16, k, want_log=False)
    else:
        g.guided_sweep(k)
    g.palette = pal
    g.optimize()
    g.error()


def child_rate(a):
    import snesimage_amd as S
    g = started(S, None, a.h)
    new = hasattr(S.OptimizedImage, "guided_run_slots")
    if a.start == "converged":
        g.run_slots(2400, seed=1, want_log=False)
    warm(g, a.k, new and a.window >= 0)
    n = 10 * C * SZ
    e0 = g.error()
    t0 = time.perf_counter()
    if a.window >= 0:
        _, _, st = g.guided_run_slots(n, a.k, window=a.window, want_log=False)
    else:
        st = dict(calls=0, accepted=0, windows=0, voided=0, scored=0, useful=0)
        for _ in range(10):
            _, s1 = g.guided_sweep(a.k)
            for key in st:
                st[key] += s1[key]
    g.sync()
    secs = time.perf_counter() - t0
    print(json.dumps(dict(leg="rate", h=a.h, start=a.start, window=a.window, calls=n, seconds=secs, calls_per_s=n / secs, stats=st, e0=e0, e1=g.error(),
                          version=S._ffi.load().snesimage_version().decode())))


def child_equal(a):
    import snesimage_amd as S
    seed = None if a.seed < 0 else a.seed
    g = started(S, seed, a.h)
    warm(g, a.k, True)
    sched = S.schedule(C, SZ, a.max_calls + 8)
    e0 = g.error()
    traj, accepted, gcalls, j = [], 0, 0, 0
    t0 = time.perf_counter()
    while j < a.max_calls and (a.seconds <= 0 or time.perf_counter() - t0 < a.seconds):
        j1 = j
        while j1 < a.max_calls and j1 - j < PIECE and sched[j1][4] == sched[j][4]:
            j1 += 1
        log, _, _ = g.run_slots(j1 - j, seed=1, first_step_id=j, state=sched[j][1:])
        traj.append((time.perf_counter() - t0, log[-1][0], j1))
        ended = sched[j1][4] != sched[j][4]
        j = j1
        if ended and a.guided:
            state = (0, 0)
            for first in range(0, C * SZ, PIECE):
                glog, state, st = g.guided_run_slots(min(PIECE, C * SZ - first), a.k, state=state)
                accepted += st["accepted"]
                gcalls += st["calls"]
                traj.append((time.perf_counter() - t0, glog[-1][0], j))
    g.sync()
    print(json.dumps(dict(leg="equal", seed=a.seed, h=a.h, guided=a.guided, e0=e0, seconds=time.perf_counter() - t0, calls=j, guided_calls=gcalls, guided_accepted=accepted, traj=traj,
                          version=S._ffi.load().snesimage_version().decode())))


def run_child(a, root, extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--k", str(a.k)] + [str(x) for x in extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        print(json.dumps({"failed": cmd[2:], "rc": r.returncode, "stderr": r.stderr[-600:]}), flush=True)
        sys.exit(1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def e_at(traj, e0, t):
    e = e0
    for s, err, _ in traj:
        if s <= t:
            e = err
    return e


def markdown(res):
    f = lambda d: "%.0f (%.0f – %.0f)" % (d["median"], d["p10"], d["p90"])
    L = ["| picture | start | leg | guided calls/s, median (10th – 90th) of %d | launch sets | voided | useful / scored | accepted |" % res["reps"], "|---|---|---|---|---|---|---|---|"]
    for r in res["rate"]:
        st = r["stats"]
        L.append("| 256 x %d | %s | %s | %s | %d | %d | %.3f | %d of %d |" % (r["h"], r["start"], r["name"], f(r["calls_per_s"]), st["windows"], st["voided"], st["useful"] / max(1, st["scored"]), st["accepted"], st["calls"]))
    L += ["", "| picture | E at start | plain s (2,400 calls) | plain: E at 25 / 50 / 100 % of its seconds | guided: E at the same seconds | guided run: scheduled + guided calls | guided calls accepted |", "|---|---|---|---|---|---|---|"]
    for r in res["equal"]:
        L.append("| %s | %.4f | %.3f | %s | %s | %d + %d | %d |" % (r["picture"], r["e0"], r["plain_seconds"], " / ".join("%.4f" % e for e in r["plain_e"]), " / ".join("%.4f" % e for e in r["guided_e"]),
                                                              r["guided_calls_scheduled"], r["guided_calls"], r["guided_accepted"]))
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_windows.json"))
    ap.add_argument("--md", default="")
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--only", choices=["rate", "equal", "both"], default="both")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--leg", choices=["rate", "equal"], default="rate")
    ap.add_argument("--h", type=int, default=256)
    ap.add_argument("--seed", type=int, default=-1)
    ap.add_argument("--start", default="kmeans")
    ap.add_argument("--window", type=int, default=0)  # -1: snesimage_guided_sweep
    ap.add_argument("--guided", type=int, default=0)
    ap.add_argument("--seconds", type=float, default=0.0)
    ap.add_argument("--max-calls", type=int, default=2400)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, a.root)
        return child_rate(a) if a.leg == "rate" else child_equal(a)
    res = dict(k=a.k, reps=a.reps, rate=[], equal=[])
    if a.only in ("rate", "both"):
        legs = [("window 0", ROOT, 0), ("window 8", ROOT, 8), ("window 64", ROOT, 64), ("sweep, this tree", ROOT, -1)] + ([("sweep, parent", os.path.abspath(a.parent), -1)] if a.parent else [])
        for h in (256, 224):
            for start in ("kmeans", "converged"):
                samples = {name: [] for name, _, _ in legs}
                for rep in range(a.reps):
                    for name, root, window in legs:  # alternating
                        r = run_child(a, root, ["--leg", "rate", "--h", h, "--start", start, "--window", window])
                        samples[name].append(r)
                        if root == ROOT:
                            res["version"] = r["version"]
                        else:
                            res["parent_version"] = r["version"]
                for name, _, _ in legs:
                    v = samples[name]
                    row = dict(h=h, start=start, name=name, calls_per_s=spread([x["calls_per_s"] for x in v]), samples=[x["calls_per_s"] for x in v], stats=v[0]["stats"], e0=v[0]["e0"], e1=v[0]["e1"])
                    print(json.dumps(row), flush=True)
                    res["rate"].append(row)
    if a.only in ("equal", "both"):
        for name, seed, h in PICTURES:
            s = -1 if seed is None else seed
            plain = run_child(a, ROOT, ["--leg", "equal", "--h", h, "--seed", s, "--guided", 0])
            T = plain["traj"][-1][0]
            guided = run_child(a, ROOT, ["--leg", "equal", "--h", h, "--seed", s, "--guided", 1, "--seconds", T, "--max-calls", 4800])
            marks = [0.25 * T, 0.5 * T, T]
            row = dict(picture=name, e0=plain["e0"], plain_seconds=T, plain_e=[e_at(plain["traj"], plain["e0"], t) for t in marks], guided_e=[e_at(guided["traj"], guided["e0"], t) for t in marks],
                       guided_seconds=guided["seconds"], guided_calls_scheduled=guided["calls"], guided_calls=guided["guided_calls"], guided_accepted=guided["guided_accepted"])
            print(json.dumps(row), flush=True)
            res["equal"].append(row)
            res["version"] = plain["version"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    md = markdown(res)
    if a.md:
        with open(a.md, "w") as f:
            f.write(md)
    print(md)


if __name__ == "__main__":
    main()
