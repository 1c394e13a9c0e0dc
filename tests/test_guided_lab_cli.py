"""The headless driver's --guided-proxy and --set-guided-proxy (DESIGN 5f'').  The misuse cases are said while parsing, before any
file or device is touched.  On the GPU a 256 x 8 run with --perceptual-palettes --guided 1 --guided-proxy cielab writes the JSON of
the model's run (guided_lab_model.cli_trajectory, whose premises tests/test_guided_lab_model.py checks on the CPU), and a --share
run with --set-guided-proxy cielab writes what the library writes when it is driven call by call."""
import os
import subprocess

import pytest

import guided_lab_model as LM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def run_cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


def test_cli_argument_rules(tmp_path):
    """The sources do not exist, so a refusal behind a file or device access would exit 1."""
    missing, out, other = str(tmp_path / "none.png"), str(tmp_path / "o.json"), str(tmp_path / "s.json")
    share = ["--share", "%s=%s" % (missing, other)]
    for args, word in [(["--guided-proxy", "cielab"], "--guided <G>"), (["--guided", "1", "--guided-proxy", "lab"], "--guided-proxy"),
                       (share + ["--set-guided-proxy", "cielab"], "--set-guided <G>"), (share + ["--set-guided", "1", "--set-guided-proxy", "ciede"], "--set-guided-proxy"),
                       (["--guided", "1", "--guided-proxy"], "--guided-proxy"), (["--guided", "1", "--guided-proxy", ""], "--guided-proxy"),
                       (["--set-guided", "1", "--set-guided-proxy", "cielab"], "--share")]:
        r = run_cli(missing, out, *args)
        assert r.returncode == 2 and "error:" in r.stderr and word in r.stderr, (args, r.stderr)
        assert "Using source image" not in r.stdout and not os.path.exists(out) and not os.path.exists(other)
    h = run_cli("--help").stderr
    assert "--guided-proxy <PROXY>" in h and "--set-guided-proxy <PROXY>" in h and h.count("[default: redmean]") == 2


@pytest.mark.gpu
def test_cli_cielab_run_writes_the_models_json(tmp_path, O):
    r = LM.cli_trajectory(O)
    c = LM.CLI_CASE
    src = tmp_path / "in.rgba"
    src.write_bytes(r["img"].tobytes())
    a, b = str(tmp_path / "a.json"), str(tmp_path / "b.json")
    common = ["-c", str(c["C"]), "-s", str(c["S"]), "--seed", "1", "--perceptual-palettes", "--guided", "1", "--guided-shortlist", str(c["K"]), "--calls", str(r["calls"])]
    out = run_cli(str(src), a, *common, "--guided-proxy", "cielab")
    assert out.returncode == 0, out.stdout + out.stderr
    n = c["C"] * c["S"]
    assert out.stdout.count("Guided sweep: %d calls, %d accepted (cielab); " % (n, sum(x["changed"] for x in r["sweep"]))) == 1, out.stdout
    assert open(a).read() == r["json"]
    red = run_cli(str(src), b, *common)
    assert red.returncode == 0, red.stdout + red.stderr
    assert red.stdout.count("Guided sweep: %d calls, " % n) == 1 and "(redmean); " in red.stdout
    assert open(b).read() != r["json"], "the proxy changed nothing: the comparison shows nothing"
    assert open(b).read() == run_and_read(tmp_path, src, common + ["--guided-proxy", "redmean"]), "redmean is the default"


def run_and_read(tmp_path, src, args):
    out = str(tmp_path / "x.json")
    r = run_cli(str(src), out, *args)
    assert r.returncode == 0, r.stdout + r.stderr
    return open(out).read()


@pytest.mark.gpu
def test_cli_share_run_with_the_sets_cielab_proxy(tmp_path, S):
    imgs = LM.frames(2, 8)  # (on two unposterised frames of this size at 2 x 3 neither proxy's sweep accepts a call)
    srcs = []
    for j, img in enumerate(imgs):
        srcs.append(tmp_path / ("in%d.rgba" % j))
        srcs[-1].write_bytes(img.tobytes())
    sched = S.schedule(2, 4, 64)
    ends = [j for j in range(63) if sched[j + 1][4] != sched[j][4]]
    calls = ends[0] + 3  # one sweep of the palette ends inside the run

    def run(tag, *extra):
        outs = [str(tmp_path / ("%s%d.json" % (tag, i))) for i in range(2)]
        r = run_cli(str(srcs[0]), outs[0], "--share", "%s=%s" % (srcs[1], outs[1]), "-c", "2", "-s", "4", "--seed", "1", "--perceptual-palettes", "--calls", str(calls), "--set-guided", "1",
                    "--set-guided-shortlist", "8", *extra)
        assert r.returncode == 0, r.stdout + r.stderr
        return [open(o).read() for o in outs], r.stdout

    a, out = run("a", "--set-guided-proxy", "cielab")
    assert out.count("Guided sweep of the set: 8 calls, ") == 1 and "accepted (cielab); " in out, out
    ctxs = [S.OptimizedImage(img, 2, 4, perceptual=True) for img in imgs]
    sp = S.SharedPalette(ctxs)
    sp.guided_proxy = "cielab"
    sp.initialize_tiles()
    sp.recalculate_palettes()
    for j in range(calls):
        method, p, i, ch, step = sched[j]
        sp.step(method, p, i, ch, 1, j, 64 if method == S.METHOD_RANDOM else 0)
        if j == ends[0]:
            sp.guided_sweep(8)
    assert [c.as_json() for c in ctxs] == a
    assert all(c.guided_proxy == "redmean" for c in ctxs)
    sp.close()
    for c in ctxs:
        c.close()
    b, out = run("b")
    assert "accepted (redmean); " in out and b != a, "the proxy changed nothing: the comparison shows nothing"
