"""What the guided calls of a shared-palette set (snesimage_shared_guided_sweep, DESIGN 5f') cost and gain, one MI355X.

    python profiles/set_guided.py [--calls 1200] [--k 16] [--rounds 5] [--out profiles/set_guided.json] [--md FILE]

Legs, every one a child process of its own under a time limit (a child that fails ends the run: nothing more is started on the
device).  Frames: synth_image(0x5EED5B00 + f, 256, 224), F = 2, 4 and 8 of them, at 8 x 15 and at 1 x 15, RGB.
  cost   from the set's k-means initialisers and 120 calls of the reference's loop through the set's slot windows; `--rounds`
         rounds over 24 slots, and in every round, slot after slot, four synchronous calls in turn, each timed by the host clock
         around the call (every one ends in a device synchronise): the generator alone (snesimage_shared_guided_candidates), a
         guided set call of K (snesimage_shared_guided_step), and snesimage_shared_step random calls of K and of 64.  The calls
         change the palette as they go; the four kinds see the same succession of states.  Median and the 10th / 90th percentile
         of each kind, after one untimed round.
  gain   from the same start, two runs: the plain schedule through the set's slot windows for `--calls` calls, and the schedule
         with one guided sweep of the set behind every sweep of the palette (cli --set-guided 1) until it has scored as many
         candidates; E of both at 25 %, 50 % and 100 % of that number (a random call counts 64, a channel call 32, a guided call
         K, per set call, whatever F), the host-clock seconds of each run, and E of both at the moment the faster one ended
         (the clock is read behind every sweep of the palette and every guided sweep).
The output is stamped with the library's source hash."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 224
COST_SHAPES = [(F, C, 15) for F in (2, 4, 8) for C in (8, 1)]
GAIN_SHAPES = [(2, 8, 15), (4, 8, 15), (8, 8, 15), (4, 1, 15)]


def started(S, F, C, Sz):
    from snesimage_amd.synth import synth_image
    ctxs = [S.OptimizedImage(synth_image(0x5EED5B00 + f, 256, H), C, Sz) for f in range(F)]
    for c in ctxs:
        c.set_chunk(64)  # (the driver's: a set call holds at most 64 candidates)
    sp = S.SharedPalette(ctxs)
    sp.initialize_tiles()
    sp.recalculate_palettes()
    return ctxs, sp


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def child_cost(a):
    import snesimage_amd as S
    ctxs, sp = started(S, a.frames, a.count, a.size)
    sp.run_slots(120, seed=1, first_step_id=0, want_log=False)
    slots = [(p, i) for p in range(a.count) for i in range(a.size)][:24]
    ms = {"generator": [], "guided_%d" % a.k: [], "random_%d" % a.k: [], "random_64": []}
    step_id = 1000
    for rnd in range(a.rounds + 1):
        for p, i in slots:
            for kind in ms:
                step_id += 1
                t0 = time.perf_counter()
                if kind == "generator":
                    sp.guided_candidates(p, i, a.k)
                elif kind.startswith("guided"):
                    sp.guided_step(p, i, a.k)
                else:
                    sp.step(S.METHOD_RANDOM, p, i, 0, 1, step_id, a.k if kind != "random_64" else 64)
                if rnd:
                    ms[kind].append(1e3 * (time.perf_counter() - t0))
    out = dict(leg="cost", frames=a.frames, h=H, count=a.count, size=a.size, k=a.k, samples=len(ms["generator"]), version=S._ffi.load().snesimage_version().decode())
    for kind, v in ms.items():
        out[kind + "_ms"] = dict(median=pct(v, 0.5), p10=pct(v, 0.1), p90=pct(v, 0.9))
    print(json.dumps(out))


def child_gain(a):
    import snesimage_amd as S
    sched = S.schedule(a.count, a.size, 4 * a.calls + 8)
    budget = sum(64 if m == 0 else 32 for m, *_ in sched[:a.calls])
    marks = [budget // 4, budget // 2, budget]
    out = dict(leg="gain", frames=a.frames, h=H, count=a.count, size=a.size, k=a.k, calls=a.calls, budget=budget)
    clocks = {}
    for name, guided in (("plain", False), ("guided", True)):
        ctxs, sp = started(S, a.frames, a.count, a.size)
        e0 = sp.error()
        t0 = time.perf_counter()
        scored, j, traj, accepted, sweeps, clock = 0, 0, [(0, e0)], 0, 0, [(0.0, e0)]
        while scored < budget:
            j1 = j
            while sched[j1][4] == sched[j][4]:
                j1 += 1
            log, _, _ = sp.run_slots(j1 - j, seed=1, first_step_id=j, state=sched[j][1:])
            for x, rec in enumerate(log):
                scored += 64 if sched[j + x][0] == 0 else 32
                traj.append((scored, rec[0]))
            clock.append((time.perf_counter() - t0, traj[-1][1]))
            j = j1
            if guided and scored < budget:
                glog, st = sp.guided_sweep(a.k)
                accepted += st["accepted"]
                sweeps += 1
                for rec in glog:
                    scored += a.k
                    traj.append((scored, rec[0]))
                clock.append((time.perf_counter() - t0, traj[-1][1]))
        secs = time.perf_counter() - t0
        at = [[e for s, e in traj if s <= mark][-1] for mark in marks]
        out[name] = dict(e0=e0, e_at_25_50_100=at, seconds=secs, optimizer_calls=j, guided_sweeps=sweeps, guided_accepted=accepted, guided_calls=sweeps * a.count * a.size)
        clocks[name] = clock
        sp.close()
        for c in ctxs:
            c.close()
    t = min(out["plain"]["seconds"], out["guided"]["seconds"])
    out["equal_clock_seconds"] = t
    for name in ("plain", "guided"):
        out[name]["e_at_equal_clock"] = [e for s, e in clocks[name] if s <= t][-1]
    print(json.dumps(out))


def run_child(a, extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--k", str(a.k), "--rounds", str(a.rounds), "--calls", str(a.calls)] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        print(json.dumps({"failed": cmd[2:], "rc": r.returncode, "stderr": r.stderr[-600:]}), flush=True)
        sys.exit(1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def markdown(res):
    L = ["| frames | geometry | generator ms | guided set call of %d ms | random set call of %d ms | random set call of 64 ms |" % (res["k"], res["k"]), "|---|---|---|---|---|---|"]
    f = lambda d: "%.3f (%.3f – %.3f)" % (d["median"], d["p10"], d["p90"])
    for r in res["cost"]:
        L.append("| %d x 256 x %d | %d x %d | %s | %s | %s | %s |" % (r["frames"], r["h"], r["count"], r["size"], f(r["generator_ms"]), f(r["guided_%d_ms" % res["k"]]), f(r["random_%d_ms" % res["k"]]), f(r["random_64_ms"])))
    L += ["", "| frames | geometry | E at start | plain E at 25 / 50 / 100 % | guided E at 25 / 50 / 100 % | plain s | guided s | E at equal clock: plain / guided (at s) | guided calls accepted |",
          "|---|---|---|---|---|---|---|---|---|"]
    for r in res["gain"]:
        p, q = r["plain"], r["guided"]
        L.append("| %d x 256 x %d | %d x %d | %.4f | %s | %s | %.2f | %.2f | %.4f / %.4f (%.2f) | %d of %d |" % (
            r["frames"], r["h"], r["count"], r["size"], p["e0"], " / ".join("%.4f" % e for e in p["e_at_25_50_100"]), " / ".join("%.4f" % e for e in q["e_at_25_50_100"]),
            p["seconds"], q["seconds"], p["e_at_equal_clock"], q["e_at_equal_clock"], r["equal_clock_seconds"], q["guided_accepted"], q["guided_calls"]))
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=1200)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_guided.json"))
    ap.add_argument("--md", default="")
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--leg", choices=["cost", "gain"], default="cost")
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--count", type=int, default=8)
    ap.add_argument("--size", type=int, default=15)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.child:
        return child_cost(a) if a.leg == "cost" else child_gain(a)
    res = dict(k=a.k, calls=a.calls, rounds=a.rounds, cost=[], gain=[])
    for F, C, Sz in COST_SHAPES:
        r = run_child(a, ["--leg", "cost", "--frames", str(F), "--count", str(C), "--size", str(Sz)])
        print(json.dumps(r), flush=True)
        res["cost"].append(r)
        res["version"] = r["version"]
    for F, C, Sz in GAIN_SHAPES:
        r = run_child(a, ["--leg", "gain", "--frames", str(F), "--count", str(C), "--size", str(Sz)])
        print(json.dumps(r), flush=True)
        res["gain"].append(r)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    md = markdown(res)
    if a.md:
        with open(a.md, "w") as f:
            f.write(md)
    print(md)


if __name__ == "__main__":
    main()
