import pytest

pytestmark = pytest.mark.gpu


def test_graft_smoke():
    import __graft_entry__ as g
    g.smoke()


def test_bench_one_gpu_line():
    """`python bench.py --full` on one GPU (a small cube, no CPU leg): one JSON line with the contract's keys, the roofline
    object measured live, the pencil and dealias extras, and a round trip inside the tolerance."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--size", "256", "--steps", "5", "--warmup", "2",
                        "--cpu-baseline", "off", "--full"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240, cwd=root)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 2 and d["dtype"] == "f64" and not d.get("degraded")
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and 0 < r["frac"] < 1 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert d["config"]["roundtrip_rel_l2"] < 1e-10
    ex = d["extras"]
    assert ex["pencil_R2CX"]["roundtrip_rel_l2"] < 1e-10
    dl = ex["dealias"]
    assert 0 < dl["ifftn_two_thirds_rule_ms"] and 0 < dl["ifftn_ms"] and 0 < dl["three_halves_rule_ifftn_fftn_pair_ms"]


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain `python bench.py` (no --full) times the headline alone: the contract's keys, exactly --steps timed steps, no
    extras and no CPU leg.  `--dump-outputs DIR` writes what the last timed step computed -- at 64^3 the whole spectrum and
    the whole round trip, as float64 -- which agree with numpy.fft, and a second run writes the same values."""
    import json
    import os
    import subprocess
    import sys
    import numpy as np
    from oracle import mpifft_oracle as orc
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = []
    for i in range(2):
        out = str(tmp_path / ("run%d" % i))
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--size", "64", "--steps", "4", "--warmup", "1",
                            "--dump-outputs", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240, cwd=root)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
        assert len(lines) == 1, lines
        d = json.loads(lines[0])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in d, k
        assert d["steps"] == 4 and d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6 * d["value"]
        assert d["extras"] == {} and d["cpu_baseline"] is None and not d.get("degraded")
        assert sorted(os.listdir(out)) == ["fftn_out.npy", "ifftn_out.npy"]
        c = np.load(os.path.join(out, "fftn_out.npy"))
        u = np.load(os.path.join(out, "ifftn_out.npy"))
        assert c.dtype == np.float64 and c.shape == (64, 64, 33, 2) and u.dtype == np.float64 and u.shape == (64, 64, 64)
        c = c[..., 0] + 1j * c[..., 1]
        assert orc.rel_l2(c, orc.slab_r2c_forward([u], np.array([64, 64, 64]))[0]) < 1e-10
        assert 0 <= u.min() and u.max() < 1 + 1e-12          # the round trip of U[0, 1) input
        runs.append((c, u))
    assert orc.rel_l2(runs[1][0], runs[0][0]) < 1e-14 and orc.rel_l2(runs[1][1], runs[0][1]) < 1e-14
