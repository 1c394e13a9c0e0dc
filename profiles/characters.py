"""What the character budget (snesimage_reduce_characters) costs and what it does to the error: the bench image cut to
256 x 224 (896 tiles), 8 x 15, RGB, one MI355X.

    python profiles/characters.py [--calls 960] [--shortlist 16] [--repeats R] [--baseline DIR] [--out profiles/characters_rgb.json]

The leg `reduce` starts from the k-means initialisers, runs `--calls` calls of the reference's loop through snesimage_run_slots,
counts the characters (U0) and reduces to 768, 640 and 512 characters in turn, or as far as eligible pairs reach.  In front of
every budget it times, at the state as it stands and with the host clock around synchronous calls (mean of 10 after 2):
  proxy_ms     snesimage_merge_shortlist(K): characters, classes, the proxy of every candidate and the shortlist;
  score_ms     snesimage_score_merges on that shortlist: K maps through the map-reading scorer;
and then the reduction itself: step_ms = its wall time / its merges.  commit_ms = step_ms - proxy_ms - score_ms is what is
left for k_merge_commit and the step's read-back; the two timed calls carry a synchronisation and a copy of their own that a
step does not pay, so commit_ms is a lower bound and can come out negative.
The leg `moves` times snesimage_score_tile_moves for K candidates at the same state (mean of 10 after 2).  --baseline DIR: a
checkout of the parent commit (its library built): `moves` also runs from it, the legs alternating, so the scoring of K
merges stands beside what the parent takes for as many candidates on the same box.
Every measurement is a child process of its own under a time limit; a child that fails ends the run: nothing more is started
on the device.  The output is stamped with the library's source hash."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGETS = (768, 640, 512)


def mean_ms(call, n=10, warm=2):
    for _ in range(warm):
        call()
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    return 1e3 * (time.perf_counter() - t0) / n


def child(a):
    sys.path.insert(0, a.root)
    import numpy as np
    import snesimage_amd as S
    from snesimage_amd import _ffi
    from snesimage_amd.synth import synth_image
    img = np.ascontiguousarray(synth_image(0x5EED0000)[:224])
    g = S.OptimizedImage(img, 8, 15)
    g.initialize_tiles()
    g.recalculate_palettes()
    g.run_slots(a.calls, seed=1, first_step_id=0, want_log=False)
    out = {"leg": a.leg, "version": _ffi.load().snesimage_version().decode(), "calls": a.calls, "shortlist": a.shortlist, "error_start": g.error()}
    if a.leg == "moves":
        rng = np.random.default_rng(1)
        tiles, tp = rng.choice(896, a.shortlist, replace=False), g.tile_palettes
        subs = [(int(tp[t]) + 1) % 8 for t in tiles]
        out["moves_ms"] = mean_ms(lambda: g.score_tile_moves(tiles, subs))
        print(json.dumps(out))
        return 0
    out["unique_start"] = g.characters()[0]
    out["budgets"] = []
    for budget in BUDGETS:
        t, b, f, _ = g.merge_shortlist(a.shortlist)
        if len(t) == 0:
            break
        rec = {"budget": budget, "proxy_ms": mean_ms(lambda: g.merge_shortlist(a.shortlist)), "score_ms": mean_ms(lambda: g.score_merges(t, b, f))}
        g.sync()
        t0 = time.perf_counter()
        recs, unique = g.reduce_characters(budget, a.shortlist)
        wall = 1e3 * (time.perf_counter() - t0)
        rec.update(merges=len(recs), unique=unique, error=g.error(), wall_ms=wall)
        if len(recs):
            rec["step_ms"] = wall / len(recs)
            rec["commit_ms"] = rec["step_ms"] - rec["proxy_ms"] - rec["score_ms"]
            rec["rank0"] = int((recs["rank"] == 0).sum())
            rec["raised"] = int((np.diff(np.concatenate([[out["budgets"][-1]["error"] if out["budgets"] else out["error_start"]], recs["error"]])) > 0).sum())
        out["budgets"].append(rec)
    print(json.dumps(out))
    return 0


def run_child(a, root, leg):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--leg", leg, "--root", root, "--calls", str(a.calls), "--shortlist", str(a.shortlist)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        print(json.dumps({"failed": cmd[2:], "rc": r.returncode, "stderr": r.stderr[-600:]}), flush=True)
        sys.exit(1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=960)
    ap.add_argument("--shortlist", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "characters_rgb.json"))
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--leg", choices=["reduce", "moves"], default="reduce")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"runs": []}
    for _ in range(a.repeats):  # the legs alternate
        for leg, root in (("reduce", ROOT), ("moves", ROOT), ("parent_moves", a.baseline)):
            if root is None:
                continue
            r = run_child(a, os.path.abspath(root), leg.replace("parent_", ""))
            r["leg"] = leg
            res["runs"].append(r)
            print(json.dumps(r), flush=True)
    res["library"] = next(r["version"] for r in res["runs"] if not r["leg"].startswith("parent_"))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
