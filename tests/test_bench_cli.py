"""bench.py's command line on one GPU: a plain run measures the headline only, `--full` the rest of the
line, and `--dump-outputs DIR` writes what the last timed step left, identically from run to run."""
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402

W, H, N = 189, 126, 4
SMALL = ["--gpus", "1", "--width", str(W), "--height", str(H), "--n-src", str(N)]
EXTRAS = ("end_to_end", "roofline_depth_to_weak", "cpu_baseline", "cpu_baseline_1core", "c2_first_init",
          "rich_texture", "sa_pass")


def _run(monkeypatch, capsys, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + SMALL + list(argv))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_and_dump(monkeypatch, capsys, tmp_path):
    """A plain run times exactly --steps steps, reports ms_per_step and none of the --full figures;
    two runs with the same arguments dump identical float arrays of every pixel."""
    dumps = []
    for d in ("a", "b"):
        line = _run(monkeypatch, capsys, "--steps", "5", "--warmup", "1", "--dump-outputs", str(tmp_path / d))
        assert line["steps"] == 5 and len(line["iter_ms"]) == 5 and line["warmup"] == 1
        assert line["value"] > 0 and line["unit"] == "Mpix/s" and line["dtype"] == "f32" and line["higher_is_better"]
        # value = pixels of the timed steps / their time, ms_per_step = that time / steps
        assert line["ms_per_step"] == pytest.approx(W * H / line["value"] / 1e3, rel=1e-3)
        assert all(line[k] is None for k in EXTRAS)
        dumps.append({f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = dumps
    assert sorted(a) == ["pixels", "planes", "selected_views"]
    assert a["planes"].shape == (W * H, 4) and a["planes"].dtype == np.float32
    assert a["selected_views"].shape == (W * H,) and a["selected_views"].dtype == np.float64
    assert np.array_equal(a["pixels"], np.arange(W * H)) and a["pixels"].dtype == np.float64
    assert np.isfinite(a["planes"]).all() and (a["planes"][:, 3] > 0).any()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


class _FakeEngine:
    """Stands in for apd_abi.Engine in dump_outputs: apd_get_results fills the caller's buffers."""
    ctx = None

    def __init__(self, n):
        self.n = n
        self.lib = self

    def apd_get_results(self, ctx, ref):
        out = ref._obj
        np.ctypeslib.as_array(out.planes, (self.n, 4))[:] = np.arange(self.n, dtype=np.float32)[:, None] % 1021
        np.ctypeslib.as_array(out.selected_views, (self.n,))[:] = np.arange(self.n) % 7
        assert not out.costs and not out.weak_info
        return 0

    def _check(self, st, what):
        assert st == 0, what


def test_dump_of_a_large_image_is_a_fixed_sample(tmp_path):
    """Above DUMP_PIXELS pixels the dump is the same sorted sample on every call, 64 MB at the most."""
    w, h = 2048, 1024 + 3
    for d in ("a", "b"):
        bench.dump_outputs(_FakeEngine(w * h), w, h, str(tmp_path / d))
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sum(v.nbytes for v in a.values()) <= 64e6 and all(v.dtype in (np.float32, np.float64) for v in a.values())
    px = a["pixels"].astype(np.int64)
    assert len(px) == bench.DUMP_PIXELS and (np.diff(px) >= 0).all() and px[0] >= 0 and px[-1] < w * h
    assert len(np.unique(px)) > 0.7 * len(px)
    assert np.array_equal(a["planes"], np.repeat((px % 1021).astype(np.float32)[:, None], 4, 1))
    assert np.array_equal(a["selected_views"], (px % 7).astype(np.float64))
    for k, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / (k + ".npy"))), k


@pytest.mark.gpu
def test_full_run_measures_the_rest(monkeypatch, capsys):
    """`--full` keeps the secondary measurements and their own switches (here: end to end and the SA
    pass on, the fixed-size C2, the rich scene and the CPU baselines off)."""
    line = _run(monkeypatch, capsys, "--steps", "3", "--warmup", "1", "--full", "--c2", "0", "--rich", "0",
                "--no-cpu-baseline")
    assert line["end_to_end"]["run_patchmatch_ms"] > 0 and line["roofline_depth_to_weak"] is not None
    assert line["sa_pass"]["mpix_s_iter"] > 0
    assert all(line[k] is None for k in ("c2_first_init", "rich_texture", "cpu_baseline", "cpu_baseline_1core"))
