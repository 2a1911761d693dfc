"""bench.py's readers of the committed profile tables (CPU): the HBM traffic of the headline kernels and the
SSAOGeneration VALU issue time come from the same workload's rocprofv3 tables under profiles/."""
import os
import sys

from conftest import ROOT

sys.path.insert(0, ROOT)


def test_pmc_traffic_of_the_headline_kernels():
    import bench
    comp, src = bench.pmc_traffic("composition_pair<true, false, 7, false>", 3840, 2160, "mesh")
    ssao, _ = bench.pmc_traffic(bench.SSAO_KERNEL, 3840, 2160, "mesh")
    assert src and os.path.exists(os.path.join(ROOT, src))
    algo = bench.algorithmic_bytes(3840, 2160, 0.0)
    # measured HBM bytes per launch: at least the algorithmic minimum's order, no more than a few times it
    assert 0.9 * algo["SSAOGeneration"] < ssao < 3.5 * algo["SSAOGeneration"]
    assert comp > 0.9 * 40.25 * 3840 * 2160
    # a template-signature change still finds the one instantiation of that kernel, or the one whose arguments extend
    # (or are extended by) the name asked for; an ambiguous name finds none
    assert bench.pmc_traffic("ssao_pipe_kernel<64, 16, 32, true, 0>", 3840, 2160, "mesh")[0] == ssao
    assert bench.pmc_traffic("composition_pair<true, false, 7, false, 1>", 3840, 2160, "mesh")[0] == comp
    assert bench.pmc_traffic("composition_pair", 3840, 2160, "mesh")[0] is None   # two instantiations in the table
    # another workload's table is not used
    assert bench.pmc_traffic(bench.SSAO_KERNEL, 1920, 1080, "mesh") == (None, None)


def test_ssao_bounds():
    """The VALU issue model of the current kernels (profiles/*valu_model.json)."""
    import bench
    vb = bench.valu_bound(bench.SSAO_KERNEL, 110.0)
    assert vb is not None and 20.0 < vb["valu_issue_us"] < 110.0
    assert abs(vb["frac_of_launch"] - vb["valu_issue_us"] / 110.0) < 1e-3
    assert bench.valu_bound("no_such_kernel", 1.0) is None


def test_dump_outputs_sample(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float32 / float64 .npy files; an image above the sample size is written as the same
    seeded pixel sample in every run, a smaller one whole."""
    import numpy as np
    import torch

    import bench

    class _Resolved:
        def __init__(self, fr):
            self.fr = fr

        def resolved(self):
            return self.fr["history_color"][1]

    H, W = 37, 53
    gen = torch.Generator().manual_seed(7)
    fr = {"output": torch.randint(0, 256, (H, W, 4), dtype=torch.uint8, generator=gen),
          "color": torch.rand((H, W, 4), generator=gen).to(torch.float16),
          "history_color": [torch.zeros(H, W, 4, dtype=torch.float16),
                            torch.rand((H, W, 4), generator=gen).to(torch.float16)],
          "auto_exposure": torch.arange(257, dtype=torch.int32)}
    fr["auto_exposure"][0] = int(np.array([0.75], np.float32).view(np.int32)[0])
    bench.dump_outputs(str(tmp_path / "whole"), fr, _Resolved(fr))
    d = {n: np.load(tmp_path / "whole" / f"{n}.npy") for n in ("output", "color", "resolved", "exposure")}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert np.array_equal(d["output"], fr["output"].reshape(-1, 4).numpy().astype(np.float32))
    assert np.array_equal(d["color"], fr["color"].reshape(-1, 4).numpy().astype(np.float32))
    assert np.array_equal(d["resolved"], fr["history_color"][1].reshape(-1, 4).numpy().astype(np.float32))
    assert d["exposure"].dtype == np.float32 and d["exposure"].tolist() == [0.75]
    # above the sample size: the same sorted, duplicate-free pixel sample twice
    monkeypatch.setattr(bench, "DUMP_SAMPLE_PIXELS", 500)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), fr, _Resolved(fr), rank=0)
    a, b = np.load(tmp_path / "a" / "output.npy"), np.load(tmp_path / "b" / "output.npy")
    assert a.shape == (500, 4) and np.array_equal(a, b)
    pick = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(H * W, 500, replace=False))
    assert len(np.unique(pick)) == 500
    assert np.array_equal(a, d["output"][pick])
    assert np.array_equal(np.load(tmp_path / "a" / "color.npy"), d["color"][pick])


def test_cpu_baseline_per_pass_medians():
    """The CPU baseline: the oracle frame timed per frame and per pass (median after a warm-up)."""
    import bench
    from helpers import sponza_inputs
    W, H = 64, 36
    g, gb = sponza_inputs(W, H, elapsed=10.0, frame_counter=2)
    host = {k: gb[k] for k in ("albedo", "emissive", "normal", "velocity", "depth", "shadow", "noise")}
    cb = bench.cpu_baseline(W, H, host, g)
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1
    assert set(cb["ms_per_pass_median"]) == {"Bloom", "SSAOGeneration", "SSAOBlur", "CloudRendering", "Composition",
                                            "GenerateLuminanceHistogram", "ResolveLuminanceHistogram",
                                            "TemporalAntiAliasing", "ToneMapping"}
    assert sum(cb["ms_per_pass_median"].values()) <= 1.5 * cb["ms_per_frame_median"] + 1.0
