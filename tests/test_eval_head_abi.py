"""CPU-side checks of the evaluation-head entry points (include/stage_hip.h "G7 evaluation head", csrc/eval_head.hip): the symbols
are exported and bound under the unchanged ABI version, the shape query answers without a GPU, and the Python layer has the two
functions the model and the prediction writer call."""
import os
import subprocess

import pytest

from conftest import ROOT

SYMBOLS = ["stage_eval_head_supported", "stage_grp_eval_head_arena_bytes", "stage_grp_eval_head_fwd", "stage_answer_spans"]


@pytest.fixture(scope="module")
def lib():
    from tvqaplus_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", ROOT, "-j8"], stdout=subprocess.DEVNULL)
    return _lib.load()


def test_symbols_exported_and_bound_under_abi_5(lib):
    from tvqaplus_amd import _lib
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.restype is _lib.SIGNATURES[name][0], name
    assert lib.stage_hip_abi_version() == 7 == _lib.ABI_VERSION


def test_shape_query_needs_no_gpu(lib):
    for Li, D, local in [(1, 4, 1), (2048, 512, 1), (2048, 128, 0)]:
        assert lib.stage_eval_head_supported(Li, D, local) == 1, (Li, D, local)
    for Li, D, local in [(0, 128, 1), (2049, 128, 1), (64, 516, 1), (64, 6, 1)]:
        assert lib.stage_eval_head_supported(Li, D, local) == 0, (Li, D, local)
    # pooled row, LayerNorm output, statistics: R * (4 D + 2) floats and the window table, each slice 256-byte aligned
    R, D = 80, 128
    need = R * (4 * D + 2) * 4 + R * 2 * 4
    assert need <= lib.stage_grp_eval_head_arena_bytes(R, D, 1) <= need + 5 * 256
    assert lib.stage_grp_eval_head_arena_bytes(R, D, 0) < lib.stage_grp_eval_head_arena_bytes(R, D, 1)


def test_python_layer_has_the_two_calls():
    from tvqaplus_amd import groups
    assert callable(groups.eval_head) and callable(groups.answer_spans)
    assert groups.eval_head_supported(2048, 512) and not groups.eval_head_supported(2049, 128)
