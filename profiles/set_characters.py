"""What the character budget of a shared-palette set (snesimage_shared_reduce_characters, DESIGN 5e'') costs and what it gains
over reducing every member on its own: frames of 256 x 224 (896 tiles each), 8 x 15, RGB, one MI355X.

    python profiles/set_characters.py [--frames 2,4,8] [--calls 240] [--shortlist 16] [--steps 24] [--baseline DIR] [--out FILE]

The leg `cost` forms a set of F frames (the bench image's generator, one seed per frame), starts from the set's k-means
initialisers, runs `--calls` calls of the reference's loop through snesimage_shared_run_slots and then times, with the host clock
around synchronous calls:
  proxy_ms   snesimage_shared_merge_shortlist(K): characters, classes, the proxy of every candidate and the shortlist (mean of
             5 after 1) — what a step recomputes, since nothing is cached between steps;
  step_ms    snesimage_shared_reduce_characters for `--steps` merges: its wall time / its merges.
proxy_share = proxy_ms / step_ms.  The timed shortlist call carries a synchronisation and a copy of its own, so the share is an
upper bound.
The legs `joint` and `separate` compare, at an equal total budget N = (U0 - F * `--steps`) rounded down to a multiple of F:
  joint      the set reduced to N characters counted together -> E (snesimage_shared_error);
  separate   what the parent commit offers: every frame on a context of its own with the set's final palette and tile palettes,
             reduced to N / F with snesimage_reduce_characters -> the sum of the members' errors, and the characters they
             hold when counted together.  --baseline DIR (a checkout of the parent commit, its library built) runs this leg
             with the parent's library; without it this tree's single-image reduction, which is the parent's code, is used.
Every measurement is a child process of its own under a time limit; a child that fails ends the run: nothing more is started
on the device.  The output is stamped with the library's source hash."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def frames(F):
    import numpy as np
    from snesimage_amd.synth import synth_image
    return [np.ascontiguousarray(synth_image(0x5EED0000 + i)[:224]) for i in range(F)]


def make_set(S, imgs, calls):
    ctxs = [S.OptimizedImage(f, 8, 15) for f in imgs]
    for c in ctxs:
        c.set_chunk(64)
    sp = S.SharedPalette(ctxs)
    sp.initialize_tiles()
    sp.recalculate_palettes()
    if calls:
        sp.run_slots(calls, seed=1, first_step_id=0, want_log=False)
    return ctxs, sp


def child(a):
    sys.path.insert(0, a.root)
    import numpy as np
    import snesimage_amd as S
    from snesimage_amd import _ffi
    out = {"leg": a.leg, "frames": a.F, "version": _ffi.load().snesimage_version().decode(), "calls": a.calls, "shortlist": a.shortlist}
    imgs = frames(a.F)
    if a.leg == "separate":  # the state the joint leg left behind, member by member, on contexts of their own
        st = json.load(open(a.state))
        E, tiles = 0.0, []
        for i, img in enumerate(imgs):
            g = S.OptimizedImage(img, 8, 15)
            g.tile_palettes = np.array(st["tile_palettes"][i], np.uint8)
            g.palette = np.array(st["palette"], np.uint8)
            g.optimize()
            recs, u = g.reduce_characters(st["budget"] // a.F, a.shortlist)
            e = g.error()
            E = e if i == 0 else E + e
            tiles += json.loads(g.as_json())["tiles"]
            g.close()
        seen = set()
        for t in tiles:  # characters counted together: equal under the four flips
            c = np.array(t, np.uint8).reshape(8, 8)
            if not any(x.tobytes() in seen for x in (c, c[:, ::-1], c[::-1], c[::-1, ::-1])):
                seen.add(c.tobytes())
        out.update(error=E, budget=st["budget"], unique_together=len(seen))
        print(json.dumps(out))
        return 0
    ctxs, sp = make_set(S, imgs, a.calls)
    U0 = sp.characters()[0]
    out.update(unique_start=U0, error_start=sp.error())
    if a.leg == "cost":
        sp.merge_shortlist(a.shortlist)
        t0 = time.perf_counter()
        for _ in range(5):
            sp.merge_shortlist(a.shortlist)
        out["proxy_ms"] = 1e3 * (time.perf_counter() - t0) / 5
        t0 = time.perf_counter()
        recs, U = sp.reduce_characters(U0 - a.steps, a.shortlist)
        wall = 1e3 * (time.perf_counter() - t0)
        out.update(merges=len(recs), unique=U, wall_ms=wall, error=sp.error())
        if len(recs):
            out["step_ms"] = wall / len(recs)
            out["proxy_share"] = out["proxy_ms"] / out["step_ms"]
            out["cross_member"] = int((recs["member"] != recs["donor_member"]).sum())
    else:  # joint: to a budget the separate reductions can be given in equal shares
        budget = (U0 - a.F * a.steps) // a.F * a.F
        recs, U = sp.reduce_characters(budget, a.shortlist)
        out.update(budget=budget, merges=len(recs), unique=U, error=sp.error(), cross_member=int((recs["member"] != recs["donor_member"]).sum()))
        with open(a.state, "w") as f:
            json.dump({"budget": budget, "palette": sp.palette.tolist(), "tile_palettes": [c.tile_palettes.tolist() for c in ctxs]}, f)
    sp.close()
    for c in ctxs:
        c.close()
    print(json.dumps(out))
    return 0


def run_child(a, root, leg, F, state):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--leg", leg, "--root", root, "--F", str(F), "--calls", str(a.calls), "--shortlist", str(a.shortlist),
           "--steps", str(a.steps), "--state", state]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        print(json.dumps({"failed": cmd[2:], "rc": r.returncode, "stderr": r.stderr[-600:]}), flush=True)
        sys.exit(1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="2,4,8")
    ap.add_argument("--calls", type=int, default=240)
    ap.add_argument("--shortlist", type=int, default=16)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_characters_rgb.json"))
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--leg", choices=["cost", "joint", "separate"], default="cost")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--F", type=int, default=2)
    ap.add_argument("--state", default=os.path.join(ROOT, "profiles", "set_characters_state.tmp.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"runs": []}
    for F in [int(v) for v in a.frames.split(",")]:
        for leg, root in (("cost", ROOT), ("joint", ROOT), ("separate", a.baseline or ROOT)):
            r = run_child(a, os.path.abspath(root), leg, F, a.state)
            r["leg"] = leg if leg != "separate" or not a.baseline else "parent_separate"
            res["runs"].append(r)
            print(json.dumps(r), flush=True)
    if os.path.exists(a.state):
        os.remove(a.state)
    res["library"] = next(r["version"] for r in res["runs"] if not r["leg"].startswith("parent_"))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
