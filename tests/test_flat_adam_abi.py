"""CPU-side checks of the flat Adam entry points (include/stage_hip.h "Flat Adam", csrc/flat_adam.hip, tvqaplus_amd/optim.py): the two
symbols are exported and bound under the unchanged ABI version, the workspace query answers without a GPU, the host-built chunk table
tiles every segment, and the optimizer class refuses what it does not implement."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

SYMBOLS = ["stage_flat_adam_ws_bytes", "stage_flat_adam_step"]
NUMELS = [1, 3, 1023, 1024, 1025, 2049, 210, 6]


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


def test_workspace_query_needs_no_gpu(lib):
    prev = 0
    for total in [1, 2, 1023, 1024, 1025, 4096, 4097, 550_000, 1 << 20, (1 << 20) + 1, 1 << 31, (1 << 33) + 5]:
        b = lib.stage_flat_adam_ws_bytes(total)
        assert b >= 4 * ((total + 1023) // 1024), total
        assert b >= prev, total
        prev = b
    assert lib.stage_flat_adam_ws_bytes(0) == 0 and lib.stage_flat_adam_ws_bytes(-7) == 0


def test_step_rejects_null_pointers_and_empty_work(lib):
    """The argument checks answer before anything touches the device: the library's shape error, no launch.
    The per-argument part (ONE bad argument, every other one plausible) belongs where no GPU is visible -- there a call that slipped
    through a regressed check fails in the launch and this test fails; with a GPU in sight it would launch on made-up addresses, so
    there every call carries a NULL pointer AND zero counts (refused by two independent checks)."""
    from tvqaplus_amd import _lib
    import ctypes
    betas = (ctypes.c_double * 2)(0.9, 0.999)
    p = 4096      # never dereferenced: every call below is refused by the checks in front of the launches
    good = [p, p, p, p, 1, p, 1, p, p, 8, 1e-3, ctypes.addressof(betas), 1e-8, 0.0, 10.0, p, 256, p, None]
    pointers, counts = (0, 1, 2, 3, 5, 7, 8, 11, 15, 17), ((9, 0), (9, -1), (6, 0), (4, 0))
    if torch.cuda.is_available():
        for i in pointers:
            bad = list(good)
            bad[i] = None
            bad[9] = bad[6] = bad[4] = 0
            assert lib.stage_flat_adam_step(*bad) == _lib.STAGE_ERR_SHAPE, i
        return
    for i in pointers:
        bad = list(good)
        bad[i] = None
        assert lib.stage_flat_adam_step(*bad) == _lib.STAGE_ERR_SHAPE, i
    for i, val in counts:
        bad = list(good)
        bad[i] = val
        assert lib.stage_flat_adam_step(*bad) == _lib.STAGE_ERR_SHAPE, (i, val)
    bad = list(good)
    bad[16] = 0
    assert lib.stage_flat_adam_step(*bad) == _lib.STAGE_ERR_WORKSPACE


def test_chunk_table_tiles_every_segment():
    from tvqaplus_amd.optim import build_chunk_table
    tab = np.asarray(build_chunk_table(NUMELS))
    assert tab.shape == (sum((n + 1023) // 1024 for n in NUMELS), 3)
    assert (tab[:, 2] >= 1).all() and (tab[:, 2] <= 1024).all()
    assert (np.diff(tab[:, 0]) >= 0).all()                       # segments in order
    for s, n in enumerate(NUMELS):
        rows = tab[tab[:, 0] == s]
        assert len(rows) == (n + 1023) // 1024, s
        pos = 0
        for _, off, ln in rows:                                   # the chunks tile [0, n) exactly, in order
            assert off == pos and off + ln <= n, (s, off, ln)
            pos += ln
        assert pos == n, s
    small = np.asarray(build_chunk_table([5, 0, 2], chunk=2))
    assert small.tolist() == [[0, 0, 2], [0, 2, 2], [0, 4, 1], [2, 0, 2]]


def test_flat_adam_rejects_what_it_does_not_implement():
    from tvqaplus_amd import parallel
    from tvqaplus_amd._lib import StageHipError
    from tvqaplus_amd.optim import FlatAdam
    params = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
    bucket = parallel.FlatGradBucket(params)
    with pytest.raises(ValueError):
        FlatAdam(bucket, amsgrad=True)
    with pytest.raises(ValueError):
        FlatAdam(bucket, maximize=True)
    for bad in (0.0, -1.0):                                     # (torch's clip_grad_norm_(0) zeroes the gradients: not offered)
        with pytest.raises(ValueError):
            FlatAdam(bucket, max_grad_norm=bad)
    with pytest.raises((ValueError, StageHipError)):            # host parameters: there is no CPU path
        FlatAdam(bucket)
