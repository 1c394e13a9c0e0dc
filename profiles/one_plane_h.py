#!/usr/bin/env python3
"""Interleaved bench runs of several builds on one MI355X, one process per run: the protocol behind BASELINE.md's
"One-plane H items" section.

usage: one_plane_h.py OUT.json [--rounds N] [--outputs] [--side] --leg NAME=TREE[,VAR=VALUE...] [--leg ...]

A leg is a source tree with its library built (TREE/bench.py is what runs) and the environment it runs under.  Every round runs
`python bench.py` and `python bench.py --gpus 1 --steps 20 --warmup 5` once per leg, in the order the legs are given.
--outputs: `--steps 20 --warmup 5 --dump-outputs` of the first two legs for plain, perceptual and dither, compared byte for byte.
--side: `--config X --steps 40 --warmup 5` of the first two legs for perceptual, dither and images.
Every run has its own time limit; the first run that fails ends the session (nothing more is started on the GPU).  OUT.json is
rewritten after every run.
"""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--leg", action="append", required=True)
ap.add_argument("--outputs", action="store_true")
ap.add_argument("--side", action="store_true")
ap.add_argument("--limit", type=int, default=240, help="seconds per run")
args = ap.parse_args()

legs = []
for spec in args.leg:
    name, rest = spec.split("=", 1)
    parts = rest.split(",")
    legs.append((name, os.path.abspath(parts[0]), dict(p.split("=", 1) for p in parts[1:])))
res = {"what": "python bench.py [args], the legs alternating on one MI355X in one session, one process per run", "legs": {n: {"tree": os.path.relpath(t), "env": e} for n, t, e in legs},
       "runs": [], "outputs": {}, "side_figures_ms_per_step": {}}


def save():
    json.dump(res, open(args.out, "w"), indent=1)


def bench(tree, env, extra):
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, "bench.py"] + extra
    p = subprocess.run(cmd, cwd=tree, env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
        res["failed"] = {"cmd": cmd, "tree": tree, "rc": p.returncode}
        save()
        sys.exit("run failed with status %d: nothing more is started" % p.returncode)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


for rnd in range(1, args.rounds + 1):
    for label, extra in (("default", []), ("s20", ["--gpus", "1", "--steps", "20", "--warmup", "5"])):
        for name, tree, env in legs:
            d = bench(tree, env, extra)
            r = {"leg": name, "round": rnd, "invocation": label, "args": extra, "env": env, "ms_per_step": d["ms_per_step"], "value": d.get("value"), "unit": d.get("unit"),
                 "steps": d.get("steps"), "warmup": d.get("warmup"), "library": d.get("library") or d.get("config", {}).get("library")}
            res["runs"].append(r)
            print("round %d %-8s %-12s %.4f ms" % (rnd, label, name, d["ms_per_step"]), flush=True)
            save()

if args.outputs or args.side:
    (na, ta, ea), (nb, tb, eb) = legs[0], legs[1]
    for cfg in ("rgb", "perceptual", "dither", "images"):
        cargs = [] if cfg == "rgb" else ["--config", cfg]
        if args.outputs and cfg != "images":
            with tempfile.TemporaryDirectory() as tmp:
                ms = {}
                for n, t, e in ((na, ta, ea), (nb, tb, eb)):
                    ms[n] = bench(t, e, cargs + ["--steps", "20", "--warmup", "5", "--dump-outputs", os.path.join(tmp, n)])["ms_per_step"]
                fa = sorted(os.path.basename(f) for f in glob.glob(os.path.join(tmp, na, "*.npy")))
                fb = sorted(os.path.basename(f) for f in glob.glob(os.path.join(tmp, nb, "*.npy")))
                same = {f: open(os.path.join(tmp, na, f), "rb").read() == open(os.path.join(tmp, nb, f), "rb").read() for f in fa}
                res["outputs"][cfg] = {"arrays": fa, "same_names": fa == fb, "identical": same, "all_identical": bool(fa) and fa == fb and all(same.values()), "ms_per_step_20": ms}
                print("outputs %-10s %s" % (cfg, res["outputs"][cfg]), flush=True)
                save()
        if args.side and cfg != "rgb":
            res["side_figures_ms_per_step"][cfg] = {n: bench(t, e, cargs + ["--steps", "40", "--warmup", "5"])["ms_per_step"] for n, t, e in ((na, ta, ea), (nb, tb, eb))}
            print("side %-10s %s" % (cfg, res["side_figures_ms_per_step"][cfg]), flush=True)
            save()
