"""What guided calls (snesimage_guided_sweep) cost and gain, one MI355X.

    python profiles/guided.py [--calls 2400] [--k 16] [--rounds 5] [--out profiles/guided.json] [--md FILE]

Legs, every one a child process of its own under a time limit (a child that fails ends the run: nothing more is started on the
device).  Shapes: synth_image() at 256 x 256 and 256 x 224, at 8 x 15 and at 1 x 15, RGB.
  cost   from the k-means initialisers and 240 calls of the reference's loop; `--rounds` rounds over 24 slots, and in every
         round, slot after slot, four synchronous calls in turn, each timed by the host clock around the call (every one ends
         in a device synchronise): the generator alone (snesimage_guided_candidates: gather, cost, select, two small copies
         back), a guided call of K (snesimage_guided_step), and snesimage_step random calls of K and of 64.  The calls change
         the palette as they go, as they do in a run; the four kinds see the same succession of states.  Median and the
         10th / 90th percentile of each kind, after one untimed round.
  gain   from the same k-means start, two runs: the plain schedule for `--calls` calls, and the schedule with one guided sweep
         behind every sweep of the palette (cli --guided 1) until it has scored as many candidates; E of both at 25 %, 50 % and
         100 % of that number (a random call counts 64, a channel call 32, a guided call K: the candidates of calls that took
         effect, not those of voided window slots), and the host-clock seconds of each run.  The bench picture and two other
         seeds.
The output is stamped with the library's source hash."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(256, 8, 15), (256, 1, 15), (224, 8, 15), (224, 1, 15)]
SEEDS = [None, 11, 12]  # None: synth_image(), the bench picture


def picture(seed, h):
    from snesimage_amd.synth import synth_image
    return synth_image(h=h) if seed is None else synth_image(seed, 256, h)


def started(S, seed, h, C, Sz):
    g = S.OptimizedImage(picture(seed, h), C, Sz)
    g.initialize_tiles()
    g.recalculate_palettes()
    return g


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def child_cost(a):
    import snesimage_amd as S
    g = started(S, None, a.h, a.count, a.size)
    g.run_slots(240, seed=1, first_step_id=0, want_log=False)
    slots = [(p, i) for p in range(a.count) for i in range(a.size)][:24]
    ms = {"generator": [], "guided_%d" % a.k: [], "random_%d" % a.k: [], "random_64": []}
    step_id = 1000
    for rnd in range(a.rounds + 1):
        for p, i in slots:
            for kind in ms:
                step_id += 1
                t0 = time.perf_counter()
                if kind == "generator":
                    g.guided_candidates(p, i, a.k)
                elif kind.startswith("guided"):
                    g.guided_step(p, i, a.k)
                else:
                    g.step(S.METHOD_RANDOM, p, i, 0, 1, step_id, a.k if kind != "random_64" else 64)
                if rnd:
                    ms[kind].append(1e3 * (time.perf_counter() - t0))
    out = dict(leg="cost", h=a.h, count=a.count, size=a.size, k=a.k, samples=len(ms["generator"]), version=S._ffi.load().snesimage_version().decode())
    for kind, v in ms.items():
        out[kind + "_ms"] = dict(median=pct(v, 0.5), p10=pct(v, 0.1), p90=pct(v, 0.9))
    print(json.dumps(out))


def child_gain(a):
    import snesimage_amd as S
    seed = None if a.image_seed < 0 else a.image_seed
    sched = S.schedule(a.count, a.size, 4 * a.calls + 8)
    budget = sum(64 if m == 0 else 32 for m, *_ in sched[:a.calls])
    marks = [budget // 4, budget // 2, budget]
    out = dict(leg="gain", h=a.h, count=a.count, size=a.size, k=a.k, image_seed=a.image_seed, calls=a.calls, budget=budget)
    for name, guided in (("plain", False), ("guided", True)):
        g = started(S, seed, a.h, a.count, a.size)
        e0 = g.error()
        t0 = time.perf_counter()
        scored, j, traj, accepted, sweeps = 0, 0, [(0, e0)], 0, 0
        while scored < budget:
            j1 = j
            while sched[j1][4] == sched[j][4]:
                j1 += 1
            log, _, _ = g.run_slots(j1 - j, seed=1, first_step_id=j, state=sched[j][1:])
            for x, rec in enumerate(log):
                scored += 64 if sched[j + x][0] == 0 else 32
                traj.append((scored, rec[0]))
            j = j1
            if guided and scored < budget:
                glog, st = g.guided_sweep(a.k)
                accepted += st["accepted"]
                sweeps += 1
                for rec in glog:
                    scored += a.k
                    traj.append((scored, rec[0]))
        g.sync()
        secs = time.perf_counter() - t0
        at = [[e for s, e in traj if s <= mark][-1] for mark in marks]
        out[name] = dict(e0=e0, e_at_25_50_100=at, seconds=secs, optimizer_calls=j, guided_sweeps=sweeps, guided_accepted=accepted, guided_calls=sweeps * a.count * a.size)
        g.close()
    print(json.dumps(out))


def run_child(a, extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--k", str(a.k), "--rounds", str(a.rounds), "--calls", str(a.calls)] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        print(json.dumps({"failed": cmd[2:], "rc": r.returncode, "stderr": r.stderr[-600:]}), flush=True)
        sys.exit(1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def markdown(res):
    L = ["| picture | geometry | generator ms | guided call of %d ms | random call of %d ms | random call of 64 ms |" % (res["k"], res["k"]), "|---|---|---|---|---|---|"]
    f = lambda d: "%.3f (%.3f – %.3f)" % (d["median"], d["p10"], d["p90"])
    for r in res["cost"]:
        L.append("| 256 x %d | %d x %d | %s | %s | %s | %s |" % (r["h"], r["count"], r["size"], f(r["generator_ms"]), f(r["guided_%d_ms" % res["k"]]), f(r["random_%d_ms" % res["k"]]), f(r["random_64_ms"])))
    L += ["", "| picture | geometry | E at start | plain E at 25 / 50 / 100 % | guided E at 25 / 50 / 100 % | plain s | guided s | guided calls accepted |", "|---|---|---|---|---|---|---|---|"]
    for r in res["gain"]:
        p, q = r["plain"], r["guided"]
        L.append("| %s 256 x %d | %d x %d | %.4f | %s | %s | %.2f | %.2f | %d of %d |" % (
            "bench" if r["image_seed"] < 0 else "seed %d" % r["image_seed"], r["h"], r["count"], r["size"], p["e0"], " / ".join("%.4f" % e for e in p["e_at_25_50_100"]),
            " / ".join("%.4f" % e for e in q["e_at_25_50_100"]), p["seconds"], q["seconds"], q["guided_accepted"], q["guided_calls"]))
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2400)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided.json"))
    ap.add_argument("--md", default="")
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--leg", choices=["cost", "gain"], default="cost")
    ap.add_argument("--h", type=int, default=256)
    ap.add_argument("--count", type=int, default=8)
    ap.add_argument("--size", type=int, default=15)
    ap.add_argument("--image-seed", type=int, default=-1)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.child:
        return child_cost(a) if a.leg == "cost" else child_gain(a)
    res = dict(k=a.k, calls=a.calls, rounds=a.rounds, cost=[], gain=[])
    for h, C, Sz in SHAPES:
        r = run_child(a, ["--leg", "cost", "--h", str(h), "--count", str(C), "--size", str(Sz)])
        print(json.dumps(r), flush=True)
        res["cost"].append(r)
        res["version"] = r["version"]
    for h, C, Sz in SHAPES:
        for seed in (SEEDS if (h, C) == (256, 8) else SEEDS[:1]):
            r = run_child(a, ["--leg", "gain", "--h", str(h), "--count", str(C), "--size", str(Sz), "--image-seed", str(-1 if seed is None else seed)])
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
