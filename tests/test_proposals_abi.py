"""No GPU: the fixed-capacity proposal layout.  ``stage.proposal_meta_host`` -- the specification of the device kernel
(csrc/proposals.hip) -- against ``stage.proposal_rows`` on random integer span tables, and the new entry point's place in the header,
the ctypes binding and the built library."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "stage_hip.h")


def random_table(N, k, Li, seed):
    """(3k + 3, N) float32 span table of valid integer spans: ranks with st <= ed < Li near the label's span or far from it,
    confidences on both sides of 0.01, some ranks empty (-1, -1, 0) as the top-K kernel leaves them."""
    rng = np.random.RandomState(seed)
    t = np.zeros((3 * k + 3, N), dtype=np.float32)
    gs = rng.randint(0, Li, N)
    ge = np.minimum(Li - 1, gs + rng.randint(0, 6, N))
    t[3 * k], t[3 * k + 1], t[3 * k + 2] = gs, ge, rng.randint(0, 5, N)
    for j in range(k):
        near = rng.rand(N) < 0.6
        st = np.where(near, np.clip(gs + rng.randint(-2, 3, N), 0, Li - 1), rng.randint(0, Li, N))
        ed = np.minimum(Li - 1, np.where(near, np.maximum(st, ge + rng.randint(-2, 3, N)), st + rng.randint(0, 6, N)))
        conf = np.where(rng.rand(N) < 0.7, rng.rand(N) * 0.5 + 0.02, rng.rand(N) * 0.009).astype(np.float32)
        empty = rng.rand(N) < 0.15
        t[3 * j] = np.where(empty, -1, st)
        t[3 * j + 1] = np.where(empty, -1, ed)
        t[3 * j + 2] = np.where(empty, 0, conf)
    return t


@pytest.mark.parametrize("N,k", [(1, 1), (3, 2), (17, 1), (40, 3), (257, 8)])
def test_proposal_meta_host_is_proposal_rows_at_capacity(N, k):
    from tvqaplus_amd.stage import proposal_meta_host, proposal_rows
    for seed, (iou, thd, extra) in enumerate([(0.5, 0.01, 3), (0.3, 0.01, 0), (0.7, 0.2, 2)]):
        table = random_table(N, k, 24, 100 * N + 10 * k + seed)
        host = table.tolist()
        src, wins, inv, tgt = proposal_rows(host, N, k, iou, thd, extra)
        meta, P = proposal_meta_host(host, N, k, iou, thd, extra)
        slots, Pmax = k + 1, (k + 1) * N
        assert meta.dtype == np.int32 and meta.shape == (5 * Pmax,)
        m_src, m_win, m_inv, m_tgt = meta[:Pmax], meta[Pmax:3 * Pmax].reshape(Pmax, 2), meta[3 * Pmax:4 * Pmax], meta[4 * Pmax:]
        # the first P rows are proposal_rows' rows; P is the sum of the per-example counts
        counts = [sum(1 for v in inv[slots * n: slots * (n + 1)] if v >= 0) for n in range(N)]
        assert P == len(src) == sum(counts) and N <= P <= Pmax
        assert m_src[:P].tolist() == src and m_win[:P].reshape(-1).tolist() == wins and m_tgt[:P].tolist() == tgt
        assert m_inv.tolist() == inv
        # the tail is row 0 with an ignored target
        assert (m_src[P:] == m_src[0]).all() and (m_win[P:] == m_win[0]).all() and (m_tgt[P:] == -100).all()
        # every row of [0, P) is named by exactly one inv entry, no entry names the tail
        named = m_inv[m_inv >= 0]
        assert sorted(named.tolist()) == list(range(P))
        # the label's span leads every example, its window is [max(0, st - extra), ed + 1 + extra)
        for n in range(N):
            r = m_inv[slots * n]
            assert m_src[r] == n and m_win[r].tolist() == [max(0, int(table[3 * k, n]) - extra), int(table[3 * k + 1, n]) + 1 + extra]


def test_capacity_reached_and_never_reached():
    from tvqaplus_amd.stage import proposal_meta_host
    N, k = 5, 2
    t = np.zeros((3 * k + 3, N), dtype=np.float32)
    t[3 * k], t[3 * k + 1], t[3 * k + 2] = 2, 5, np.arange(N) % 5
    for j in range(k):
        t[3 * j], t[3 * j + 1], t[3 * j + 2] = 2, 5 - j, 0.5           # IoU 1 and 3 / 4
    meta, P = proposal_meta_host(t.tolist(), N, k, 0.5, 0.01, 3)
    assert P == (k + 1) * N and (meta[4 * P:] >= 0).all()                  # every slot full: no padding row
    t[2::3][:k] = 0.001
    meta, P = proposal_meta_host(t.tolist(), N, k, 0.5, 0.01, 3)
    Pmax = (k + 1) * N
    assert P == N and (meta[4 * Pmax + N:] == -100).all()
    assert meta[3 * Pmax:4 * Pmax].reshape(N, k + 1).tolist() == [[n, -1, -1] for n in range(N)]


def test_double_comparisons_of_the_specification():
    """np.float32(0.01) is below the double 0.01: rejected; its next float up is kept.  An IoU exactly at the threshold is kept."""
    from tvqaplus_amd.stage import proposal_meta_host
    lo = np.float32(0.01)
    hi = np.nextafter(lo, np.float32(1))
    assert float(lo) < 0.01 <= float(hi)
    t = np.array([[4, 4], [5, 5], [lo, hi], [4, 4], [5, 5], [1, 2]], dtype=np.float32)
    _, P = proposal_meta_host(t.tolist(), 2, 1, 0.5, 0.01, 3)
    assert P == 3
    t = np.array([[4], [4], [0.5], [4], [5], [0]], dtype=np.float32)      # inter 1 / union 2
    assert proposal_meta_host(t.tolist(), 1, 1, 0.5, 0.01, 3)[1] == 2
    t = np.array([[0], [2], [0.5], [0], [9], [0]], dtype=np.float32)      # inter 3 / union 10
    assert proposal_meta_host(t.tolist(), 1, 1, 0.3, 0.01, 3)[1] == 2
    t = np.array([[0], [1], [0.5], [0], [9], [0]], dtype=np.float32)      # inter 2 / union 10
    assert proposal_meta_host(t.tolist(), 1, 1, 0.3, 0.01, 3)[1] == 1


def test_symbol_in_header_binding_and_library():
    import ctypes
    from tvqaplus_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+stage_proposal_meta\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, "include/stage_hip.h does not declare stage_proposal_meta"
    args = [a.strip() for a in m.group(1).split(",")]
    res, argtypes = _lib.SIGNATURES["stage_proposal_meta"]
    assert res is ctypes.c_int and len(args) == len(argtypes) == 9
    for a, t in zip(args, argtypes):
        assert (t is ctypes.c_void_p) == ("*" in a) and (t is ctypes.c_int) == ("*" not in a), (a, t)
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", ROOT, "-j8"], stdout=subprocess.DEVNULL)
    lib = _lib.load()
    assert hasattr(lib, "stage_proposal_meta")
    hdr = open(HEADER).read()
    assert int(re.search(r"#define STAGE_HIP_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == lib.stage_hip_abi_version() == 7


def test_shape_limits_are_answered_before_any_launch():
    """K outside 1 .. STAGE_TOPK_MAX, N <= 0 and a NULL pointer return STAGE_ERR_SHAPE without touching a device."""
    import ctypes
    from tvqaplus_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", ROOT, "-j8"], stdout=subprocess.DEVNULL)
    lib = _lib.load()
    thd = (ctypes.c_double * 2)(0.5, 0.01)
    fake = ctypes.c_void_p(4096)        # never dereferenced: every call below is declined first
    for N, K in [(4, 0), (4, _lib.STAGE_TOPK_MAX + 1), (0, 1), (-3, 2), (2 ** 30, 8)]:
        assert lib.stage_proposal_meta(fake, N, K, thd, 3, fake, fake, fake, None) == _lib.STAGE_ERR_SHAPE, (N, K)
    assert lib.stage_proposal_meta(None, 4, 1, thd, 3, fake, fake, fake, None) == _lib.STAGE_ERR_SHAPE
    assert lib.stage_proposal_meta(fake, 4, 1, None, 3, fake, fake, fake, None) == _lib.STAGE_ERR_SHAPE
    assert lib.stage_proposal_meta(fake, 4, 1, thd, -1, fake, fake, fake, None) == _lib.STAGE_ERR_SHAPE


def test_option_is_off_by_default_and_read_from_opt():
    import contextlib
    import io
    from tvqaplus_amd.stage import STAGE
    from tvqaplus_amd.synth import make_opt
    with contextlib.redirect_stdout(io.StringIO()):
        a = STAGE(make_opt(hsz=16, embedding_size=8, vfeat_size=8))
        opt = make_opt(hsz=16, embedding_size=8, vfeat_size=8)
        opt.device_proposals = True
        b = STAGE(opt)
    assert a.device_proposals is False and b.device_proposals is True and a.last_proposals is None
