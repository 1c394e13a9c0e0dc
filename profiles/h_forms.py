#!/usr/bin/env python3
"""Interleaved bench runs of the parent build and this one under each SNES_H_FORMS mask on one MI355X, one process per run:
the protocol behind profiles/h_forms_ab.json (the H pass in a kernel per form; profiles/v2_pairs.py with the legs fixed).

usage: h_forms.py OUT.json --parent TREE [--rounds N] [--main] [--outputs] [--side] [--masks M,M] [--parent-twice]

TREE is a checkout of the parent commit with its library built (TREE/bench.py is what runs there).  The legs, in this order:
parent, new (the default mask), bit1, bit2, bit4 (SNES_H_FORMS = 1, 2, 4) and forms0 (SNES_H_FORMS=0: the parent's launches).
--main:    every round runs `python bench.py` and `python bench.py --gpus 1 --steps 20 --warmup 5` once per leg and keeps
           ms_per_step.
--outputs: `--steps 20 --warmup 5 --dump-outputs` of parent and new for rgb, perceptual and dither; every array compared with
           numpy.array_equal.
--side:    `--config perceptual`, `--config dither`, `--batch 8192`, `--batch 64` and `--config images` of parent and new,
           twice, alternating.
Every run has its own time limit; the first run that fails ends the session (nothing more is started on the GPU).  OUT.json is
read if it exists, so that the parts may be taken in several sessions, and rewritten after every run.
"""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--parent", required=True)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--main", action="store_true")
ap.add_argument("--outputs", action="store_true")
ap.add_argument("--side", action="store_true")
ap.add_argument("--masks", default="", help="further legs of this build, e.g. 3,6")
ap.add_argument("--parent-twice", action="store_true", help="a second parent leg at the end of every round: the same-build spread inside a round")
ap.add_argument("--limit", type=int, default=240, help="seconds per run")
args = ap.parse_args()

parent = os.path.abspath(args.parent)
legs = [("parent", parent, {}), ("new", HERE, {}), ("bit1", HERE, {"SNES_H_FORMS": "1"}), ("bit2", HERE, {"SNES_H_FORMS": "2"}),
        ("bit4", HERE, {"SNES_H_FORMS": "4"}), ("forms0", HERE, {"SNES_H_FORMS": "0"})]
legs += [("mask%s" % m, HERE, {"SNES_H_FORMS": m}) for m in args.masks.split(",") if m]
if args.parent_twice:
    legs.append(("parent_b", parent, {}))
if os.path.exists(args.out):
    res = json.load(open(args.out))
else:
    res = {"what": "python bench.py [args], the legs alternating on one MI355X, one process per run",
           "legs": {n: {"tree": "parent" if t == parent else "this", "env": e} for n, t, e in legs}, "runs": [], "outputs": {}, "side": []}


def save():
    json.dump(res, open(args.out, "w"), indent=1)


def bench(tree, env, extra):
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, "bench.py"] + extra
    p = subprocess.run(cmd, cwd=tree, env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
        res["failed"] = {"cmd": cmd, "leg_env": env, "rc": p.returncode}
        save()
        sys.exit("run failed with status %d: nothing more is started" % p.returncode)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


def record(where, name, env, label, extra, d, **more):
    r = dict({"leg": name, "invocation": label, "args": extra, "env": env, "ms_per_step": d["ms_per_step"],
              "steps": d.get("steps"), "library": d.get("library")}, **more)
    where.append(r)
    print("%-10s %-8s %.4f ms" % (label, name, r["ms_per_step"]), flush=True)
    save()


if args.main:
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
                             ("batch8192", ["--batch", "8192", "--steps", "100", "--warmup", "5"]), ("batch64", ["--batch", "64", "--steps", "400", "--warmup", "10"]),
                             ("images", ["--config", "images", "--steps", "40", "--warmup", "5"])):
            for name, tree, env in legs[:2]:
                record(res["side"], name, env, label, extra, bench(tree, env, extra), round=rnd)
