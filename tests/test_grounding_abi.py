"""CPU-side checks of the grounding meter's C ABI (include/stage_hip.h "Grounding meter", csrc/grounding.hip): the four symbols are
declared, bound and exported under the unchanged ABI version, the two queries answer without a GPU, and the argument checks answer
before any launch."""
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

from tvqaplus_amd import grounding as G

SYMBOLS = ["stage_grounding_supported", "stage_grounding_bytes", "stage_grounding_reset", "stage_grounding_update"]


@pytest.fixture(scope="module")
def lib():
    from tvqaplus_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", ROOT, "-j8"], stdout=subprocess.DEVNULL)
    return _lib.load()


def test_header_binding_and_exports_agree_under_abi_5(lib):
    import ctypes
    from tvqaplus_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stage_hip.h")).read(), flags=re.S)
    kinds = {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t}
    for name in SYMBOLS:
        m = re.search(r"\b(int|size_t)\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        args = [ctypes.c_void_p if "*" in a else kinds[re.sub(r"\b\w+$", "", a.strip()).strip()] for a in m.group(2).split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert argtypes == args and res is kinds[m.group(1)], name
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is res, name
    assert lib.stage_hip_abi_version() == 7 == _lib.ABI_VERSION


def test_queries_need_no_gpu(lib):
    for Lqa, Lr, ok in [(40, 25, 1), (1, 1, 1), (64, 64, 1), (65, 25, 0), (40, 65, 0), (0, 25, 0), (40, 0, 0), (-1, -1, 0)]:
        assert lib.stage_grounding_supported(Lqa, Lr) == ok, (Lqa, Lr)
    assert lib.stage_grounding_bytes(0) == G.HEAD_BYTES == 64
    for cap in [1, 2, 3, 255, 4096, 100_001, (1 << 31) + 3]:
        assert lib.stage_grounding_bytes(cap) == G.HEAD_BYTES + 8 * cap
    assert lib.stage_grounding_bytes(-1) == 0


def test_calls_reject_bad_arguments_before_any_launch(lib):
    """As tests/test_meter_abi.py: the one-bad-argument part runs where no GPU is visible (a call that slipped through a regressed
    check fails in the launch there); with a GPU in sight every call carries a NULL buffer AND a bad size."""
    from tvqaplus_amd import _lib
    E = _lib.STAGE_ERR_SHAPE
    p = 4096      # never dereferenced: every call below is refused by the checks in front of the launch
    upd = [p, 16, p, 1000, p, 200, p, 3, p, 10, p, 10, 40, 25, 0.2, 0.5, None]

    def with_(**kw):
        out = list(upd)
        for i, v in kw.items():
            out[int(i[1:])] = v
        return out

    if torch.cuda.is_available():
        assert lib.stage_grounding_reset(None, -1, None) == E
        assert lib.stage_grounding_update(*with_(_0=None, _13=65)) == E
        return
    assert lib.stage_grounding_reset(None, 8, None) == E
    assert lib.stage_grounding_reset(p, -1, None) == E
    assert lib.stage_grounding_reset(p + 4, 8, None) == E                    # not 8-byte aligned
    for bad in (dict(_0=None), dict(_0=p + 2), dict(_1=-1), dict(_2=None), dict(_3=-1), dict(_4=None), dict(_4=p + 4), dict(_5=-1),
                dict(_6=None), dict(_6=p + 4), dict(_7=-1), dict(_8=None), dict(_9=-1), dict(_10=None), dict(_11=-1), dict(_12=0),
                dict(_12=65), dict(_13=0), dict(_13=65)):
        assert lib.stage_grounding_update(*with_(**bad)) == E, bad
    assert lib.stage_grounding_update(*with_(_7=0)) == 0                     # no task: no launch
