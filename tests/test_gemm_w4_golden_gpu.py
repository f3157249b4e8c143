"""The 4-wave GEMM kernels (csrc/gemm_w4.h) reproduce, bit for bit, the outputs recorded in
tests/golden/gemm_w4_digests.json before the bf16 and fp8 copies of the schedule were unified. For
these kernels the output is a pure function of the inputs (fixed accumulation order; the column
sums are folded in a fixed order under PZ_DETERMINISTIC, the default), so equality is the condition."""
import hashlib
import json
import os

import pytest
import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "gemm_w4_digests.json")

# name -> (kind, M, N, K); inputs come from CPU generators seeded as the case records
CASES = {
    "var40_store_2steps": ("bf16_store", 4096, 4096, 128),    # two K steps: only the peeled tail runs
    "var40_store_5steps": ("bf16_store", 4096, 4096, 320),    # the loop body, an odd step count
    "var40_bwd_mask_5steps": ("bf16_bwd_mask", 4096, 4096, 320),
    "var43_store": ("fp8_fwd_store", 4096, 4096, 2048),
}


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def run_case(name):
    """-> (record of the inputs, {output name: sha256}, PF.gemm_last_kernel())"""
    kind, M, N, K = CASES[name]
    out = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    if kind == "fp8_fwd_store":
        seed, sa, sb = K, 0.25, 1.0 / 32
        g = torch.Generator(device="cpu").manual_seed(seed)
        x8 = (torch.randn(M, K, generator=g) * 4).to(DEV).to(torch.float8_e4m3fn)
        w8 = (torch.randn(K, N, generator=g) * 2).to(DEV).to(torch.float8_e4m3fn)  # [in, out]
        PF.gemm(x8, True, w8, False, out, scale_a=torch.tensor([sa], device=DEV), scale_b=torch.tensor([sb], device=DEV))
        return {"seed": seed, "scale_a": sa, "scale_b": sb}, {"out": _sha(out)}, PF.gemm_last_kernel()
    seed = M + K
    g = torch.Generator(device="cpu").manual_seed(seed)
    gz = torch.randn(M, K, generator=g).to(DEV, torch.bfloat16)
    wt = torch.randn(N, K, generator=g).to(DEV, torch.bfloat16)
    if kind == "bf16_store":
        PF.gemm(gz, True, wt, True, out)
        return {"seed": seed}, {"out": _sha(out)}, PF.gemm_last_kernel()
    p, epi_seed = 0.2, (7, 9)
    mask = PF.relu_mask_pack(torch.randn(M, N, generator=g).to(DEV) > 0)
    cs = torch.zeros(N, device=DEV)
    epi = PF.epi_spec(act=PF.ACT_RELU, drop_pre=1, drop_post=2, p=p, seed=epi_seed)
    PF.gemm(gz, True, wt, True, out, colsum=cs, mode=PF.EPI_BWD, epi=epi, mask=mask)
    return ({"seed": seed, "p": p, "epi_seed": list(epi_seed)}, {"out": _sha(out), "colsum": _sha(cs)},
            PF.gemm_last_kernel())


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_gemm_w4_output_digests(native_lib, golden, name):
    kind, M, N, K = CASES[name]
    want = golden[name]
    assert (want["kind"], want["M"], want["N"], want["K"]) == (kind, M, N, K)
    inputs, digests, kernel = run_case(name)
    assert inputs == want["inputs"]
    assert kernel.startswith("w4/var43/" if kind == "fp8_fwd_store" else "w4/var40/"), kernel
    assert digests == want["sha256"]
