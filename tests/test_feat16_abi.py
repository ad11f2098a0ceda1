"""CPU-side checks of the half-precision feature entry points (csrc/feat16.hip, include/stage_hip.h): the library builds and exports
them, the host-side predicate says which rows the kernels take, and the size queries need no GPU."""
import os
import subprocess

import pytest

from conftest import ROOT

F32, F16, BF16 = 0, 1, 2        # include/stage_hip.h: STAGE_DT_F32 / STAGE_DT_F16 / STAGE_DT_BF16

SYMBOLS = ["stage_feat16_supported", "stage_feat16_ln_fwd", "stage_feat16_ln_bwd_ws_bytes", "stage_feat16_ln_bwd",
           "stage_grp_input_mlp_arena_bytes", "stage_grp_input_mlp_fwd", "stage_grp_input_mlp_bwd"]


@pytest.fixture(scope="module")
def lib():
    from tvqaplus_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", ROOT, "-j8"], stdout=subprocess.DEVNULL)
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    from tvqaplus_amd import _lib
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert (_lib.STAGE_DT_F32, _lib.STAGE_DT_F16, _lib.STAGE_DT_BF16) == (F32, F16, BF16)
    hdr = open(os.path.join(ROOT, "include", "stage_hip.h")).read()
    assert "#define STAGE_DT_F32 0" in hdr and "#define STAGE_DT_F16 1" in hdr and "#define STAGE_DT_BF16 2" in hdr
    assert lib.stage_hip_abi_version() == 7


def test_supported_truth_table(lib):
    for dt in (F16, BF16):
        for K0 in (4, 300, 768, 1024):
            assert lib.stage_feat16_supported(K0, dt) == 1, (K0, dt)
        for K0 in (6, 1028, 0, -4, 2):
            assert lib.stage_feat16_supported(K0, dt) == 0, (K0, dt)
    for dt in (0, 3, -1, 16):                        # 0 is float32 in the Python layer: never a code of these entry points
        assert lib.stage_feat16_supported(768, dt) == 0, dt


def test_size_queries_need_no_gpu(lib):
    for K0 in (4, 300, 768, 1024):
        ws = lib.stage_feat16_ln_bwd_ws_bytes(K0)
        assert ws >= 2 * K0 * 4                       # at least one [2][K0] partial row
        assert ws == lib.stage_ln_bwd_ws_bytes(K0)    # the input-MLP group's backward scratch (sized for the fp32 kernel) serves both
    for M, K0, H, D in ((1, 4, 8, 8), (67, 300, 300, 128), (1031, 768, 300, 128), (96000, 300, 300, 128), (240000, 768, 300, 128)):
        old_l2 = lib.stage_grp_input_mlp_arena_bytes(M, K0, H, D, 1, F32)
        for dt in (F16, BF16):
            for l2 in (0, 1):
                new = lib.stage_grp_input_mlp_arena_bytes(M, K0, H, D, l2, dt)
                assert 0 < new <= old_l2 - M * K0 * 4, (M, K0, new, old_l2)       # no normalised image
                assert new == lib.stage_grp_input_mlp_arena_bytes(M, K0, H, D, 0, F32)
