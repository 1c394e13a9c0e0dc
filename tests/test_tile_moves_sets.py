"""Objective-scored tile moves on shared-palette sets (snesimage_shared_tile_sweep) and in the headless driver
(--tile-moves), against the model of tests/tile_model.py over the CPU oracle."""
import json
import os
import subprocess

import numpy as np
import pytest

from tile_model import REL_ERR, assert_log_matches, model_tile_sweep

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


def frames(F, H, variant=0, seed=0x5EED5700):
    from snesimage_amd.synth import synth_image
    return [synth_image(seed + i, 256, H, variant) for i in range(F)]


def oracle_members(O, imgs, ctxs, count, size, **flags):
    out = []
    for f, c in zip(imgs, ctxs):
        o = O.OracleImage(f, count, size, **flags)
        o.tile_palettes = c.tile_palettes
        o.palette = c.palette
        o.optimize()
        out.append(o)
    return out


@pytest.mark.parametrize("flags", [{}, {"dither": True}], ids=["rgb", "dither"])
def test_shared_tile_sweep_equals_the_model_member_by_member(O, flags):
    """Three members: every call is decided on the member's own error; shared_error is the member-order sum; the set steps
    and runs its slot windows from the new tile palettes as the model does."""
    import snesimage_amd as S
    count, size, n = 2, 3, 40
    imgs = frames(3, 64, 1)
    ctxs = [S.OptimizedImage(f, count, size, device=0, **flags) for f in imgs]
    for c in ctxs:
        c.set_chunk(64)
    sp = S.SharedPalette(ctxs)
    sp.initialize_tiles()
    sp.recalculate_palettes()
    sp.run(4, seed=2, n_random=8)
    oms = oracle_members(O, imgs, ctxs, count, size, **flags)
    log, stats = sp.tile_sweep(3, n)
    assert log.shape == (3, n) and stats["calls"] == 3 * n and stats["windows"] < stats["calls"]
    accepted = 0
    for i, o in enumerate(oms):
        want = model_tile_sweep(o, 3, n, count)
        assert_log_matches(log[i], want)
        accepted += sum(ch for _, _, ch in want)
        assert np.array_equal(ctxs[i].tile_palettes, o.tile_palettes) and np.array_equal(ctxs[i].palette_map, o.palette_map)
    assert stats["accepted"] == accepted and accepted > 0
    E = 0.0
    for o in oms:
        E = E + o.error()
    assert abs(sp.error() - E) <= REL_ERR * E
    # the set goes on from there: one call and a short run of slot windows against the summed oracle
    pal = oms[0].palette
    seed, n_random = 9, 8
    got, _, _ = sp.run_slots(6, seed=seed, first_step_id=0, n_random=n_random)
    for j, (method, p, idx, ch, _) in enumerate(O.schedule(count, size, 6)):
        cand = O.random_candidates(seed, j, n_random)
        inc = 0.0
        for o in oms:
            inc = inc + o.error()
        Ek = None
        for o in oms:
            e = o.score_candidates(p, idx, cand)
            Ek = e if Ek is None else Ek + e
        k = int(np.argmin(Ek))
        if Ek[k] < inc:
            pal[p * size + idx] = cand[k]
            for o in oms:
                o.palette = pal
                o.optimize()
        want_e = Ek[k] if Ek[k] < inc else inc
        assert np.array_equal(got[j][2], pal[p * size + idx]) and abs(got[j][0] - want_e) <= REL_ERR * want_e, j
    sp.step(S.METHOD_RANDOM, 0, 0, 0, 1, 100, 8)
    sp.close()
    for c in ctxs:
        c.close()


def run_model(O, img, count, size, calls, ncand, seed, tile_every, flags=None):
    o = O.OracleImage(img, count, size, **(flags or {}))
    o.initialize_tiles()
    o.recalculate_palettes()
    moves = []
    sched = O.schedule(count, size, calls + 1)
    ntile = 32 * (img.shape[0] // 8)
    for i, (method, p, idx, ch, step) in enumerate(sched[:calls]):
        o.step(method, p, idx, ch, seed, i, ncand if method == 0 else 0)
        if tile_every and sched[i + 1][4] != step and sched[i + 1][4] % tile_every == 0:
            moves.append(sum(c for _, _, c in model_tile_sweep(o, 0, ntile, count)))
    return o, moves


def test_cli_tile_moves_matches_the_model(tmp_path, O):
    """--tile-moves 1 on a 2 x 3 run of two sweeps (calls 6 and 12 end a sweep): after each, one tile sweep over the image.
    The JSON is the model's; without the flag it is what it always was."""
    img = frames(1, 64, 0, seed=0x5EED5800)[0]
    src = tmp_path / "in.rgba"
    src.write_bytes(img.tobytes())
    count, size, calls, ncand = 2, 3, 14, 8
    common = [str(src), "-c", str(count), "-s", str(size), "--calls", str(calls), "--candidates", str(ncand), "--seed", "5"]
    out = tmp_path / "out.json"
    r = cli(common[0], str(out), *common[1:], "--tile-moves", "1")
    assert r.returncode == 0, r.stdout + r.stderr
    o, moves = run_model(O, img, count, size, calls, ncand, 5, 1)
    assert len(moves) == 2 and moves[0] > 0
    assert [int(l.split("Moved ")[1].split()[0]) for l in r.stdout.splitlines() if "Moved " in l] == moves
    assert out.read_text() == o.as_json()
    logged = [l.split("Current Error: ")[1] for l in r.stdout.splitlines() if "Current Error: " in l]
    assert abs(float(logged[-1]) - o.error()) <= 1e-9 * o.error()
    plain = tmp_path / "plain.json"
    r2 = cli(common[0], str(plain), *common[1:])
    assert r2.returncode == 0 and "Moved " not in r2.stdout
    o2, _ = run_model(O, img, count, size, calls, ncand, 5, 0)
    assert plain.read_text() == o2.as_json() and plain.read_text() != out.read_text()
    # --resume continues from the moved tiles
    again = tmp_path / "again.json"
    r3 = cli(common[0], str(again), "-c", str(count), "-s", str(size), "--resume", str(out), "--tile-moves", "1")
    assert r3.returncode == 0 and again.read_text() == out.read_text()
    o.close()
    o2.close()


def test_cli_tile_moves_with_share(tmp_path, O):
    """Two frames, one palette, one tile sweep after the second sweep of the palette: the files equal the model's sweep,
    frame by frame, from the state the same run leaves without the flag; the palette is the same in both."""
    imgs = frames(2, 64, 1, seed=0x5EED5900)
    for i, f in enumerate(imgs):
        (tmp_path / ("f%d.rgba" % i)).write_bytes(f.tobytes())
    args = [str(tmp_path / "f0.rgba"), str(tmp_path / "o0.json"), "--share", "%s=%s" % (tmp_path / "f1.rgba", tmp_path / "o1.json"),
            "-c", "2", "-s", "3", "--calls", "12", "--candidates", "8"]
    r = cli(*args, "--tile-moves", "2")
    assert r.returncode == 0, r.stdout + r.stderr
    moved = [int(l.split("Moved ")[1].split()[0]) for l in r.stdout.splitlines() if "Moved " in l]
    assert len(moved) == 1 and moved[0] > 0
    outs = [json.loads((tmp_path / ("o%d.json" % i)).read_text()) for i in range(2)]
    assert outs[0]["palette"] == outs[1]["palette"]
    pal16 = outs[0]["palette"]
    rgb5 = np.array([[v & 31, (v >> 5) & 31, (v >> 10) & 31] for p in range(2) for v in pal16[16 * p + 1:16 * p + 4]], np.uint8)
    # the model: the same run without the flag gives the state before the sweep (12 calls = two sweeps of the palette, the
    # tile sweep follows the second); the model's sweep from there must end in the files written with the flag
    r0 = cli(args[0], str(tmp_path / "p0.json"), "--share", "%s=%s" % (tmp_path / "f1.rgba", tmp_path / "p1.json"), *args[4:])
    assert r0.returncode == 0, r0.stdout + r0.stderr
    total = 0
    for i, f in enumerate(imgs):
        before = json.loads((tmp_path / ("p%d.json" % i)).read_text())
        assert before["palette"] == pal16  # the sweep leaves the palette alone
        o = O.OracleImage(f, 2, 3)
        tp = np.zeros(1024, np.uint8)
        tp[:len(before["tile_palettes"])] = before["tile_palettes"]
        o.tile_palettes = tp
        o.palette = rgb5
        o.optimize()
        total += sum(c for _, _, c in model_tile_sweep(o, 0, 256, 2))
        assert o.as_json() == (tmp_path / ("o%d.json" % i)).read_text(), i
        o.close()
    assert total == moved[0]
