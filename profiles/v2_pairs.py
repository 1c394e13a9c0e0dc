#!/usr/bin/env python3
"""Interleaved bench runs of several builds on one MI355X, one process per run: the protocol behind profiles/v2_pairs_ab.json
(two candidates per wave in the V pass of scale 0; profiles/one_plane_h.py with the dominant launch's duration, the batch sizes
and the outputs compared as arrays).

usage: v2_pairs.py OUT.json [--rounds N] [--outputs] [--side] --leg NAME=TREE[,VAR=VALUE...] [--leg ...]

A leg is a source tree with its library built (TREE/bench.py is what runs) and the environment it runs under.  Every round runs
`python bench.py` and `python bench.py --gpus 1 --steps 20 --warmup 5` once per leg, in the order the legs are given, and keeps
ms_per_step and roofline.avg_launch_ms (k_sparse_v2 in company).
--outputs: `--steps 20 --warmup 5 --dump-outputs` of the first two legs for rgb, perceptual and dither; every array compared
           with numpy.array_equal.
--side:    `--config perceptual`, `--config dither`, `--batch 8192` and `--batch 64` of every leg, twice, alternating.
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

import numpy as np

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
res = {"what": "python bench.py [args], the legs alternating on one MI355X in one session, one process per run",
       "legs": {n: {"tree": os.path.relpath(t), "env": e} for n, t, e in legs}, "runs": [], "outputs": {}, "side": []}


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


def record(where, name, env, label, extra, d, **more):
    r = dict({"leg": name, "invocation": label, "args": extra, "env": env, "ms_per_step": d["ms_per_step"],
              "avg_launch_ms": d.get("roofline", {}).get("avg_launch_ms"), "dominant": d.get("roofline", {}).get("kernel"),
              "steps": d.get("steps"), "library": d.get("library")}, **more)
    where.append(r)
    print("%-10s %-12s %.4f ms  launch %s" % (label, name, r["ms_per_step"], r["avg_launch_ms"]), flush=True)
    save()


for rnd in range(1, args.rounds + 1):
    for label, extra in (("default", []), ("s20", ["--gpus", "1", "--steps", "20", "--warmup", "5"])):
        for name, tree, env in legs:
            record(res["runs"], name, env, label, extra, bench(tree, env, extra), round=rnd)

if args.outputs:
    (na, ta, ea), (nb, tb, eb) = legs[0], legs[1]
    for cfg in ("rgb", "perceptual", "dither"):
        cargs = [] if cfg == "rgb" else ["--config", cfg]
        with tempfile.TemporaryDirectory() as tmp:
            for n, t, e in ((na, ta, ea), (nb, tb, eb)):
                bench(t, e, cargs + ["--steps", "20", "--warmup", "5", "--dump-outputs", os.path.join(tmp, n)])
            fa = sorted(os.path.basename(f) for f in glob.glob(os.path.join(tmp, na, "*.npy")))
            fb = sorted(os.path.basename(f) for f in glob.glob(os.path.join(tmp, nb, "*.npy")))
            same = {f: bool(np.array_equal(np.load(os.path.join(tmp, na, f)), np.load(os.path.join(tmp, nb, f)))) for f in fa if f in fb}
            res["outputs"][cfg] = {"arrays": fa, "same_names": fa == fb, "array_equal": same, "all_identical": bool(fa) and fa == fb and all(same.values())}
            print("outputs %-10s %s" % (cfg, res["outputs"][cfg]), flush=True)
            save()

if args.side:
    for rnd in (1, 2):
        for label, extra in (("perceptual", ["--config", "perceptual", "--steps", "40", "--warmup", "5"]), ("dither", ["--config", "dither", "--steps", "40", "--warmup", "5"]),
                             ("batch8192", ["--batch", "8192", "--steps", "100", "--warmup", "5"]), ("batch64", ["--batch", "64", "--steps", "400", "--warmup", "10"])):
            for name, tree, env in legs:
                record(res["side"], name, env, label, extra, bench(tree, env, extra), round=rnd)
