"""Host-side checks of the exact-arithmetic GEMM cases (gemm_exact_cases.py): no kernel is launched.

  * Every bf16 and MX-fp8 case is planned on the kernel its GPU test expects (ste_gemm_kernel,
    ste_gemm_kernel_name, ste_gemm_mx8_kernel are host-only), under the lowered plan thresholds where
    the case asks for them, taking CU = 256 where the plan depends on the CU count.
  * One representative case per group: the generator's operands meet the 2^24 precondition and torch's
    fp32 matmul on the CPU equals fp64 exactly, i.e. the reference alone satisfies the zero tolerance.
"""
import contextlib
import ctypes as C

import pytest
import torch

from gemm_exact_cases import (BY_ID, CASES, CU_DEFAULT, case_m, epi_of, expected_kernel, handover_m, logical_operands,
                              plan_args)


@pytest.fixture(scope="module")
def ops():
    from speech_transcript_embeddings_amd import _lib, ops as _ops
    if not _lib.LIB_PATH.exists():
        pytest.fail("libste.so not built — run __graft_entry__.build()")
    return _ops


def test_case_tables():
    assert len(CASES) == len(BY_ID) > 250
    assert {c.group for c in CASES} == {1, 2, 3, 4, 5, 6, 8}   # group 7 (the quantiser) has no GEMM plan
    m = handover_m(CU_DEFAULT)
    assert 2 * ((m + 255) // 256) > CU_DEFAULT and m % 256 == 200


@pytest.mark.parametrize("cid", [c.id for c in CASES if c.kind != "f32"])
def test_planned_kernel(ops, cid):
    from speech_transcript_embeddings_amd import _lib
    c = BY_ID[cid]
    want_id, want = expected_kernel(c)
    a = plan_args(c, CU_DEFAULT)
    with (ops.bench_gemm_plan() if c.low else contextlib.nullcontext()):
        if c.kind == "mx8":
            eight = int(_lib.fn("ste_gemm_mx8_kernel")(C.byref(a), int(bool(epi_of(c.epi).get("q8")))))
            assert eight == int(c.path == "mx8ph"), (cid, eight)
        else:
            assert int(_lib.fn("ste_gemm_kernel")(C.byref(a))) == want_id, cid
            assert ops.gemm_kernel_name(a) == want, cid
    assert ops.gemm_plan_min_tiles() == (240, 240)   # the thresholds are back at their defaults


@pytest.mark.parametrize("cid", ["g1-300x261x320-kk-f32-plain", "g2a-plain_f32", "g3-256x256x9024-dw",
                                 "g4-2048x264x2624-gen_fwd", "g5-136x261x200-mk-f32-plain",
                                 "g6-8ph-bf16-257x264x384", "g8-64x72x1028-kk-split"])
def test_reference_is_exact_in_fp32(cid):
    c = BY_ID[cid]
    _, a, b, _ = logical_operands(c, CU_DEFAULT, "cpu")
    unit = 0.25 if c.kind == "mx8" else 1.0
    bound = torch.bmm(a.abs(), b.abs().transpose(1, 2)).amax().item() / unit
    assert bound < 2 ** 24, bound
    ref = torch.bmm(a, b.transpose(1, 2))
    got = torch.bmm(a.float(), b.float().transpose(1, 2))
    assert torch.equal(got.double(), ref)
    assert case_m(c, CU_DEFAULT) == a.shape[1]
