"""``bench.py --dump-outputs``: the writer itself, on CPU tensors (no GPU needed)."""
import types

import numpy as np
import torch

import bench


def _model(dtype):
    g = torch.Generator().manual_seed(0)
    return types.SimpleNamespace(params=[torch.randn(300, 70, generator=g, dtype=torch.float64).to(dtype),
                                         torch.randn(70, generator=g, dtype=torch.float64).to(dtype)])


def test_dump_writes_costs_ratios_and_params(tmp_path):
    m = _model(torch.bfloat16)
    bench._dump_outputs(str(tmp_path / "a"), m, [2.5, 2.25], [0.125, None])
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["costs.npy", "param_00.npy", "param_01.npy",
                                                                 "weight_upd_ratio.npy"]
    costs = np.load(tmp_path / "a" / "costs.npy")
    assert costs.dtype == np.float64 and costs.tolist() == [2.5, 2.25]
    ratios = np.load(tmp_path / "a" / "weight_upd_ratio.npy")
    assert ratios.dtype == np.float64 and ratios[0] == 0.125 and np.isnan(ratios[1])
    for i, p in enumerate(m.params):  # under the cap: whole, in order, exact (bf16 -> fp32 is exact)
        got = np.load(tmp_path / "a" / f"param_{i:02d}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, p.float().reshape(-1).numpy())


def test_dump_samples_large_params_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_PARAM_BYTES", 2 * 8 * 1000)  # 1000 fp64 elements per parameter
    m = _model(torch.float64)
    bench._dump_outputs(str(tmp_path / "a"), m, [1.0], None)
    bench._dump_outputs(str(tmp_path / "b"), m, [1.0], None)
    assert not (tmp_path / "a" / "weight_upd_ratio.npy").exists()
    a0, b0 = np.load(tmp_path / "a" / "param_00.npy"), np.load(tmp_path / "b" / "param_00.npy")
    assert a0.dtype == np.float64 and a0.shape == (1000,) and np.array_equal(a0, b0)
    flat = m.params[0].reshape(-1).numpy()
    assert np.isin(a0, flat).all() and len(np.unique(a0)) > 900  # a spread sample of its values
    assert np.array_equal(np.load(tmp_path / "a" / "param_01.npy"), m.params[1].numpy())  # 70 <= 1000: whole
