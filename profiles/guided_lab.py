"""What the CIELAB proxy of guided calls (snesimage_set_guided_proxy, DESIGN 5f'') costs and gains against the redmean proxy, on
the bench picture with --perceptual-palettes, one MI355X.

    python profiles/guided_lab.py [--calls 1200] [--k 16] [--rounds 3] [--parent DIR] [--out profiles/guided_lab.json] [--md FILE]

Legs, every one a child process of its own under a time limit (a child that fails ends the run: nothing more is started on the
device).  synth_image() at 256 x 256, perceptual, at 8 x 15 and at the worst case 1 x 15 (every pixel in one subpalette).
  cost   from the k-means initialisers and 240 calls of the reference's loop; `--rounds` rounds over the first 24 slots, and in
         every round, slot after slot, synchronous calls in turn, each timed by the host clock around the call (every one ends in
         a device synchronise): the generator alone (snesimage_guided_candidates) and a guided call of K (snesimage_guided_step)
         under REDMEAN and then under CIELAB, on the same context, the proxy switched between them.  Median and the 10th / 90th
         percentile of each kind after one untimed round.  Then whole sweeps (snesimage_guided_sweep), the two proxies in turn,
         `--rounds` each after one untimed pair.  --parent DIR: a tree of the parent commit, built (its snesimage_amd package is
         imported from there by children of their own); its redmean calls are timed by the same code, its children alternating
         with this tree's.
  gain   from the same k-means start, the schedule with one guided sweep behind every sweep of the palette (cli --guided 1) for
         `--calls` scheduled calls, once per proxy: E at 25 %, 50 % and 100 % of the calls, the guided calls accepted per sweep
         and the host-clock seconds.
The output is stamped with the library's source hash."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 15), (1, 15)]


def started(S, C, Sz):
    from snesimage_amd.synth import synth_image
    g = S.OptimizedImage(synth_image(), C, Sz, perceptual=True)
    g.initialize_tiles()
    g.recalculate_palettes()
    return g


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def spread(v):
    return dict(median=pct(v, 0.5), p10=pct(v, 0.1), p90=pct(v, 0.9))


def child_cost(a):
    import snesimage_amd as S
    g = started(S, a.count, a.size)
    g.run_slots(240, seed=1, first_step_id=0, want_log=False)
    proxies = ["redmean", "cielab"] if hasattr(S.OptimizedImage, "guided_proxy") else ["redmean"]  # (the parent commit has one)
    slots = [(p, i) for p in range(a.count) for i in range(a.size)][:24]
    ms = {kind + "_" + proxy: [] for proxy in proxies for kind in ("generator", "guided")}
    for rnd in range(a.rounds + 1):
        for p, i in slots:
            for proxy in proxies:
                if len(proxies) > 1:
                    g.guided_proxy = proxy
                for kind in ("generator", "guided"):
                    t0 = time.perf_counter()
                    if kind == "generator":
                        g.guided_candidates(p, i, a.k)
                    else:
                        g.guided_step(p, i, a.k)
                    if rnd:
                        ms[kind + "_" + proxy].append(1e3 * (time.perf_counter() - t0))
    sweeps = {proxy: [] for proxy in proxies}
    for rnd in range(a.rounds + 1):
        for proxy in proxies:
            if len(proxies) > 1:
                g.guided_proxy = proxy
            t0 = time.perf_counter()
            g.guided_sweep(a.k)
            if rnd:
                sweeps[proxy].append(1e3 * (time.perf_counter() - t0))
    out = dict(leg="cost", count=a.count, size=a.size, k=a.k, samples=len(ms["generator_redmean"]), version=S._ffi.load().snesimage_version().decode())
    for kind, v in ms.items():
        out[kind + "_ms"] = spread(v)
    for proxy, v in sweeps.items():
        out["sweep_" + proxy + "_ms"] = spread(v)
    print(json.dumps(out))


def child_gain(a):
    import snesimage_amd as S
    sched = S.schedule(a.count, a.size, a.calls + 8)
    marks = [a.calls // 4, a.calls // 2, a.calls]
    out = dict(leg="gain", count=a.count, size=a.size, k=a.k, calls=a.calls)
    for proxy in ("redmean", "cielab"):
        g = started(S, a.count, a.size)
        g.guided_proxy = proxy
        e0 = g.error()
        t0 = time.perf_counter()
        j, traj, accepted, sweeps = 0, [(0, e0)], [], 0
        while j < a.calls:
            j1 = j
            while j1 < a.calls and sched[j1][4] == sched[j][4]:
                j1 += 1
            log, _, _ = g.run_slots(j1 - j, seed=1, first_step_id=j, state=sched[j][1:])
            for x, rec in enumerate(log):
                traj.append((j + x + 1, rec[0]))
            ended = sched[j1][4] != sched[j][4]
            j = j1
            if ended:
                glog, st = g.guided_sweep(a.k)
                accepted.append(st["accepted"])
                sweeps += 1
                traj.append((j, glog[-1][0]))
        g.sync()
        secs = time.perf_counter() - t0
        at = [[e for s, e in traj if s <= mark][-1] for mark in marks]
        out[proxy] = dict(e0=e0, e_at_25_50_100=at, e_end=g.error(), seconds=secs, guided_sweeps=sweeps, guided_accepted=accepted, guided_calls_per_sweep=a.count * a.size)
        g.close()
    print(json.dumps(out))


def run_child(a, root, extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--k", str(a.k), "--rounds", str(a.rounds), "--calls", str(a.calls)] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        print(json.dumps({"failed": cmd[2:], "rc": r.returncode, "stderr": r.stderr[-600:]}), flush=True)
        sys.exit(1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def markdown(res):
    f = lambda d: "%.3f (%.3f – %.3f)" % (d["median"], d["p10"], d["p90"])
    L = ["| tree | geometry | proxy | generator ms | guided call of %d ms | guided sweep ms |" % res["k"], "|---|---|---|---|---|---|"]
    for r in res["cost"]:
        for proxy in ("redmean", "cielab"):
            if "generator_%s_ms" % proxy in r:
                L.append("| %s | %d x %d | %s | %s | %s | %s |" % (r["tree"], r["count"], r["size"], proxy, f(r["generator_%s_ms" % proxy]), f(r["guided_%s_ms" % proxy]), f(r["sweep_%s_ms" % proxy])))
    L += ["", "| geometry | proxy | E at start | E at 25 / 50 / 100 %% of %d calls | guided calls accepted per sweep | s |" % res["calls"], "|---|---|---|---|---|---|"]
    for r in res["gain"]:
        for proxy in ("redmean", "cielab"):
            q = r[proxy]
            L.append("| %d x %d | %s | %.4f | %s | %s of %d | %.2f |" % (r["count"], r["size"], proxy, q["e0"], " / ".join("%.4f" % e for e in q["e_at_25_50_100"]),
                                                                      ", ".join(str(n) for n in q["guided_accepted"]), q["guided_calls_per_sweep"], q["seconds"]))
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=1200)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_lab.json"))
    ap.add_argument("--md", default="")
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--leg", choices=["cost", "gain"], default="cost")
    ap.add_argument("--count", type=int, default=8)
    ap.add_argument("--size", type=int, default=15)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, a.root)
        return child_cost(a) if a.leg == "cost" else child_gain(a)
    res = dict(k=a.k, calls=a.calls, rounds=a.rounds, cost=[], gain=[])
    trees = [("this", ROOT)] + ([("parent", os.path.abspath(a.parent))] if a.parent else [])
    for C, Sz in SHAPES:
        for rep in range(2 if a.parent else 1):  # twice, alternating, when there is a parent to compare with: the spread between equal runs
            for tree, root in trees:
                r = run_child(a, root, ["--leg", "cost", "--count", str(C), "--size", str(Sz)])
                r["tree"] = tree
                print(json.dumps(r), flush=True)
                res["cost"].append(r)
                if tree == "this":
                    res["version"] = r["version"]
    r = run_child(a, ROOT, ["--leg", "gain", "--count", "8", "--size", "15"])
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
