"""-m gpu: the encoder group (G2: csrc/groups.hip, stage_grp_encoder_{fwd,bwd}) in every form -- dense (S, L, D) rows unpooled, pooled
with LayerNorm + max fused (D = 128) and unfused (D = 64, 16), zero to three conv layers; the compact rows of a ragged layout pooled
(statement rows) and unpooled (a context stream) -- each with dropout off and on, against the same chain spelled out as per-kernel
calls: the dense one through the tvqaplus_amd.ops wrappers as STAGE._encoder_block's per-op branch spells it, the ragged one through the
library's stage_ln_dwconv_rag_* / stage_rag_fill_pooled / stage_ln_masked_max_rag_* (small autograd Functions below) around
ops.linear / ops.layernorm.  The group only sequences those kernels, with the same arguments and workspace sizes, so ``out``, ``dx``
and every parameter gradient are held to torch.equal, and so are two runs of the group.

x is a view into the middle of a buffer whose surroundings are NaN.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_hip_ragged_kernels import EPS, NEG32, _block_params, _ok, _p, _st, _statement_layout

pytestmark = pytest.mark.gpu

P_DROP = 0.1
SEEDS = (0x51DE5EED0001, 0x1234ABCD5EED)      # one per even conv layer
PAD = 64                                      # floats of NaN in front of and behind x (the view stays 256-byte aligned)
MASK_ROWS = 41 * 101                          # 4141 = 4096 + 45: the 1x1 convs + ReLU run on the streaming kernel with the ReLU bit mask
DENSE_SHAPES = [(3, 5, 16),                   # fewer rows than a wave handles
                (7, 37, 128),                 # a row tail over several blocks
                (41, 101, 64), (41, 101, 128)]


@pytest.fixture(scope="module")
def lib(hip_device):
    from tvqaplus_amd import _lib
    return _lib.load()


def test_mask_shape_is_the_threshold(lib):
    for S, L, D in DENSE_SHAPES:
        assert lib.stage_gemm_mask_supported(S * L, D, D) == (1 if S * L == MASK_ROWS else 0)
    for D in (64, 128):
        assert lib.stage_gemm_mask_supported(4096, D, D) == 1 and lib.stage_gemm_mask_supported(4095, D, D) == 0


def _nan_framed(t, dev):
    buf = torch.full((t.numel() + 2 * PAD,), float("nan"), device=dev)
    buf[PAD: PAD + t.numel()] = t.reshape(-1).to(dev)
    return buf[PAD: PAD + t.numel()].view(t.shape)


def _compare(what, run_group, run_chain):
    """group == chain and group == group, bit for bit: out, dx, every parameter gradient; dropout off and on"""
    for p in (0.0, P_DROP):
        ref = run_chain(p)
        got, again = run_group(p), run_group(p)
        torch.cuda.synchronize()
        assert got[0].shape == ref[0].shape and all(bool(torch.isfinite(t).all()) for t in got)
        d = [float((a.reshape(-1) - b.reshape(-1)).abs().max()) for a, b in zip(got, ref)]
        print("%s p=%.1f max|group - chain|: out %.3e dx %.3e grads %s" % (what, p, d[0], d[1], " ".join("%.3e" % v for v in d[2:])))
        for i, (a, b, a2) in enumerate(zip(got, ref, again)):
            assert torch.equal(a.reshape(-1), b.reshape(-1)), (what, p, i, d[i])
            assert torch.equal(a, a2), (what, p, i, "two runs differ")
    return got


def _grads(out, x, ps, dout):
    return [out.detach()] + list(torch.autograd.grad(out, [x] + ps, dout))


# =====================================================================================================================
# dense rows
# =====================================================================================================================
def _dense_chain(x, pe, pm, p, ps, n_conv):
    """STAGE._encoder_block's per-op branch (no self-attention)"""
    from tvqaplus_amd import ops
    _, L, D = x.shape
    pending, cur, period = x, pe, L
    for i in range(n_conv):
        q, drop = ps[6 * i: 6 * i + 6], i % 2 == 0
        h, cur = ops.ln_dwconv(pending, q[0], q[1], q[2], q[3], p=p if drop else 0.0, seed=SEEDS[i // 2] if drop else 0, res=cur,
                               res_period=period)
        period = 0
        pending = ops.linear(h, q[4], q[5], relu=True)
    g, b = ps[-2:]
    if pm is not None and period == 0 and ops.ln_masked_max_supported(pending, L, D):
        return ops.ln_masked_max(pending, cur, g, b, pm)
    y, _ = ops.layernorm(pending, g, b, res=cur, res_period=period)
    return y if pm is None else ops.masked_max(y, pm)


@pytest.mark.parametrize("k", [5, 7])
@pytest.mark.parametrize("n_conv", [0, 1, 2, 3])
@pytest.mark.parametrize("pooled", [0, 1], ids=["rows", "pooled"])
@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dense_forms_equal_the_spelled_out_chain(hip_device, lib, shape, pooled, n_conv, k):
    from tvqaplus_amd import groups
    from tvqaplus_amd.stage import _PositionTable
    dev = hip_device
    S, L, D = shape
    if pooled and n_conv:
        assert lib.stage_ln_masked_max_supported(L, D) == (1 if D == 128 else 0)       # fused at 128, the unfused pair at 64 and 16
    g = torch.Generator().manual_seed(1000 * S + 10 * D + n_conv + k)
    _, vals = _block_params(D, k, n_conv, g)
    vals = [v.to(dev) for v in vals]
    x = _nan_framed(torch.randn(S, L, D, generator=g), dev).requires_grad_(True)
    pe = _PositionTable.table(L + 3, D).to(dev)
    pm = None
    if pooled:       # prefix masks of every length from 1, one row with holes
        pm = (torch.arange(L)[None, :] < (1 + torch.arange(S) * 7 % L)[:, None]).float()
        pm[S - 1, ::2] = 0.0
        pm = pm.to(dev)
    dout = torch.randn((S, D) if pooled else (S, L, D), generator=g).to(dev)

    def run(fn):
        ps = [v.detach().clone().requires_grad_(True) for v in vals]
        return _grads(fn(ps), x, ps, dout)

    got = _compare("dense %s pooled=%d n_conv=%d k=%d" % (shape, pooled, n_conv, k),
                   lambda p: run(lambda ps: groups.encoder_block(x, pe, pm, k, p, SEEDS[:(n_conv + 1) // 2], ps)),
                   lambda p: run(lambda ps: _dense_chain(x, pe, pm, p, ps, n_conv)))
    assert got[1].shape == x.shape


# =====================================================================================================================
# ragged rows
# =====================================================================================================================
class _LnDwconvRag(torch.autograd.Function):
    """stage_ln_dwconv_rag_{fwd,bwd} on the sequences of ``lay``: (h, x + res + pe); the gradient of the sum is added into dx"""
    @staticmethod
    def forward(ctx, lib, lay, x, res, pe, gamma, beta, w, bias, p, seed):
        U, D = x.shape
        k = w.shape[-1]
        h, s = torch.empty_like(x), torch.empty_like(x)
        mean, rstd = torch.empty(U, device=x.device), torch.empty(U, device=x.device)
        _ok(lib.stage_ln_dwconv_rag_fwd(x.data_ptr(), _p(res), _p(pe), s.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w.data_ptr(),
                                        bias.data_ptr(), h.data_ptr(), mean.data_ptr(), rstd.data_ptr(), lay.seq.data_ptr(), lay.S, lay.Lqa,
                                        D, k, EPS, p, seed, _st()), "stage_ln_dwconv_rag_fwd")
        ctx.save_for_backward(s, mean, rstd, gamma, beta, w)
        ctx.cfg = (lib, lay, p, seed)
        ctx.set_materialize_grads(False)
        return h, s

    @staticmethod
    def backward(ctx, dh, ds):
        s, mean, rstd, gamma, beta, w = ctx.saved_tensors
        lib, lay, p, seed = ctx.cfg
        (U, D), k = s.shape, w.shape[-1]
        dx, dg, db, dw, dbias = torch.empty_like(s), torch.empty_like(gamma), torch.empty_like(gamma), torch.empty_like(w), torch.empty_like(gamma)
        wsb = lib.stage_ln_dwconv_bwd_ws_bytes(D, k)
        ws = torch.empty(wsb, dtype=torch.uint8, device=s.device)
        _ok(lib.stage_ln_dwconv_rag_bwd(dh.data_ptr(), s.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                        w.data_ptr(), dx.data_ptr(), _p(ds), dg.data_ptr(), db.data_ptr(), dw.data_ptr(), dbias.data_ptr(),
                                        lay.seq.data_ptr(), lay.S, lay.Lqa, D, k, p, seed, ws.data_ptr(), wsb, _st()), "stage_ln_dwconv_rag_bwd")
        return None, None, dx, (dx if ctx.needs_input_grad[3] else None), None, dg, db, dw, dbias, None, None


class _LnMaskedMaxRag(torch.autograd.Function):
    """stage_rag_fill_pooled + stage_ln_masked_max_rag_{fwd,bwd}: (lay.out_rows, K) dense"""
    @staticmethod
    def forward(ctx, lib, lay, x, res, gamma, beta, qmask):
        U, K = x.shape
        Rd = lay.out_rows
        out, idx = torch.empty(Rd, K, device=x.device), torch.empty(Rd, K, dtype=torch.int32, device=x.device)
        s, mean, rstd = torch.empty_like(x), torch.empty(U, device=x.device), torch.empty(U, device=x.device)
        _ok(lib.stage_rag_fill_pooled(out.data_ptr(), idx.data_ptr(), Rd, K, _st()), "stage_rag_fill_pooled")
        _ok(lib.stage_ln_masked_max_rag_fwd(x.data_ptr(), res.data_ptr(), s.data_ptr(), gamma.data_ptr(), beta.data_ptr(), qmask.data_ptr(),
                                            out.data_ptr(), idx.data_ptr(), mean.data_ptr(), rstd.data_ptr(), lay.seq.data_ptr(), lay.S,
                                            lay.Lqa, K, EPS, _st()), "stage_ln_masked_max_rag_fwd")
        ctx.save_for_backward(s, mean, rstd, gamma, idx, qmask)
        ctx.cfg = (lib, lay)
        return out

    @staticmethod
    def backward(ctx, dout):
        s, mean, rstd, gamma, idx, qmask = ctx.saved_tensors
        lib, lay = ctx.cfg
        U, K = s.shape
        dx, dg, db = torch.empty_like(s), torch.empty_like(gamma), torch.empty_like(gamma)
        wsb = lib.stage_ln_bwd_ws_bytes(K)
        ws = torch.empty(wsb, dtype=torch.uint8, device=s.device)
        _ok(lib.stage_ln_masked_max_rag_bwd(dout.data_ptr(), idx.data_ptr(), qmask.data_ptr(), s.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                            gamma.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), lay.rowinfo.data_ptr(), U, K,
                                            ws.data_ptr(), wsb, _st()), "stage_ln_masked_max_rag_bwd")
        return None, None, dx, dx, dg, db, None


def _ragged_chain(lib, lay, x, pe, qmask, p, ps, n_conv):
    from tvqaplus_amd import ops
    pending, cur = x, None
    for i in range(n_conv):
        q, drop = ps[6 * i: 6 * i + 6], i % 2 == 0
        h, cur = _LnDwconvRag.apply(lib, lay, pending, cur, pe if i == 0 else None, q[0], q[1], q[2], q[3], p if drop else 0.0,
                                    SEEDS[i // 2] if drop else 0)
        pending = ops.linear(h, q[4], q[5], relu=True)
    g, b = ps[-2:]
    if qmask is None:
        return ops.layernorm(pending, g, b, res=cur)[0]
    return _LnMaskedMaxRag.apply(lib, lay, pending, cur, g, b, qmask)


def _ragged_case(dev, lib, what, lay, qmask, pe_rows, k, n_conv, seed0):
    from tvqaplus_amd import groups
    from tvqaplus_amd.stage import _PositionTable
    D, U = 128, lay.U
    g = torch.Generator().manual_seed(seed0)
    _, vals = _block_params(D, k, n_conv, g)
    vals = [v.to(dev) for v in vals]
    x = _nan_framed(torch.randn(U, D, generator=g), dev).requires_grad_(True)
    pe = _PositionTable.table(pe_rows, D).to(dev)
    qm = None if qmask is None else qmask.to(dev)
    dout = torch.randn(lay.out_rows if qmask is not None else U, D, generator=g).to(dev)

    def run(fn):
        ps = [v.detach().clone().requires_grad_(True) for v in vals]
        return _grads(fn(ps), x, ps, dout)

    got = _compare("%s U=%d S=%d n_conv=%d k=%d" % (what, U, lay.S, n_conv, k),
                   lambda p: run(lambda ps: groups.encoder_block_rag(x, pe, qm, lay, k, p, SEEDS[:(n_conv + 1) // 2], ps)),
                   lambda p: run(lambda ps: _ragged_chain(lib, lay, x, pe, qm, p, ps, n_conv)))
    assert got[1].shape == x.shape
    return got[0]


def _dead_rows_hold_the_fill(out, tab, lay):
    live = torch.zeros(lay.out_rows, dtype=torch.bool)
    live[[int(r[3]) for r in tab.seq]] = True
    assert not bool(live.all()) and bool((out.cpu()[~live] == NEG32).all())


@pytest.mark.parametrize("n_conv", [1, 2])
@pytest.mark.parametrize("Lqa", [13, 40])
def test_ragged_pooled_equals_the_spelled_out_chain(hip_device, lib, Lqa, n_conv):
    tab, lay, qmask = _statement_layout(hip_device, Lqa)
    assert lib.stage_gemm_mask_supported(lay.U, 128, 128) == 0
    out = _ragged_case(hip_device, lib, "ragged pooled Lqa=%d" % Lqa, lay, qmask, Lqa, 5, n_conv, 100 + Lqa + n_conv)
    _dead_rows_hold_the_fill(out, tab, lay)


def test_ragged_pooled_on_the_mask_path_equals_the_spelled_out_chain(hip_device, lib):
    """N, NA, Li, Lqa = 2, 5, 12, 40 with all but two frames live: more than 4096 compact rows"""
    from tvqaplus_amd import ragged
    N, NA, Li, Lqa = 2, 5, 12, 40
    qa = np.zeros((N * NA, Lqa), bool)
    for gi, l in enumerate([40, 36, 38, 40, 30, 40, 37, 40, 40, 33]):
        qa[gi, :l] = True
    qa[3, [2, 7, 11]] = False
    fl = np.ones((N, Li), bool)
    fl[1, [5, 9]] = False
    tab = ragged.RaggedTables(qa.reshape(N, NA, Lqa), fl, 4)
    lay = ragged.RaggedLayout(tab, hip_device)
    assert lay.U >= 4096 and lib.stage_gemm_mask_supported(lay.U, 128, 128) == 1
    out = _ragged_case(hip_device, lib, "ragged pooled mask path", lay, torch.from_numpy(qa.astype(np.float32)), Lqa, 5, 2, 77)
    _dead_rows_hold_the_fill(out, tab, lay)


@pytest.mark.parametrize("n_conv", [1, 2])
def test_ragged_unpooled_on_a_context_layout_equals_the_spelled_out_chain(hip_device, lib, n_conv):
    from tvqaplus_amd import ragged
    L, halo = 60, 6
    lens = np.array([[0, 1, 24, 25, 54, 60, 13, 0], [60, 2, 37, 25, 1, 48, 24, 9]])       # (kept lengths 7, 30, 31, 60: the chunk edge)
    lay = ragged.CtxLayout(ragged.CtxTables(lens, L, halo), hip_device)
    _ragged_case(hip_device, lib, "ragged unpooled", lay, None, L, 7, n_conv, 300 + n_conv)


# =====================================================================================================================
# refusals
# =====================================================================================================================
def test_refusals_come_before_a_launch(hip_device, lib):
    """every refusal of include/stage_hip.h, both directions: its code comes back and out, arena, tmp and the gradients keep their
    sentinels.  Every buffer is sized for W-wide layers: a call that was not refused stays inside."""
    from tvqaplus_amd import _lib
    dev = hip_device
    tab, lay, qmask = _statement_layout(dev, 13)
    U, W, NC = lay.U, 1028, 2
    assert U > 3 * 5 + 1
    SHAPE, WORKSPACE = _lib.STAGE_ERR_SHAPE, _lib.STAGE_ERR_WORKSPACE
    stream = _st()
    ones = torch.ones(max(W * W, (U + 1) * W), device=dev)             # x, pe, the mask and every parameter
    qm = qmask.to(dev)
    big = int(lib.stage_grp_encoder_arena_bytes(U + 1, lay.out_rows, W, NC, 1, 0))
    tmp_b = int(lib.stage_grp_encoder_bwd_tmp_bytes(U + 1, W, 9, 1, 0))
    ptrs = lambda t: (ctypes.c_void_p * 64)(*[t.data_ptr()] * 64)
    seeds = (ctypes.c_ulonglong * 8)(3, 4, 5, 6, 7, 8, 9, 10)
    dense = dict(T=None, pooled=0, rows=15, cap=15, S=3, out_rows=3, L=5, D=16, n_conv=NC, k=5)
    ragged = dict(T=lay.T, pooled=1, rows=U, cap=U, S=lay.S, out_rows=lay.out_rows, L=13, D=128, n_conv=NC, k=5)

    def call(base, arena_bytes=None, tmp_bytes=None, fwd=True, **over):
        a = dict(base, **over)
        out = torch.full((max(lay.out_rows, U + 1) * W,), -7.0, device=dev)
        grad = torch.full((W * W,), -7.0, device=dev)                   # every gradient, and dx
        arena = torch.full((big,), 0x5A, dtype=torch.uint8, device=dev)
        tmp = torch.full((tmp_b,), 0x5A, dtype=torch.uint8, device=dev)
        flags = (ctypes.c_int * 16)()
        mask = None if not a["pooled"] else (qm if a["T"] is not None else ones).data_ptr()
        ab = big if arena_bytes is None else arena_bytes
        dims = (a["rows"], a["cap"], a["S"], a["out_rows"], a["L"], a["D"], a["n_conv"], a["k"], 0.1, seeds, stream)
        rcs = []
        if fwd:
            rcs.append(lib.stage_grp_encoder_fwd(ones.data_ptr(), ones.data_ptr(), mask, ptrs(ones), out.data_ptr(), a["T"], arena.data_ptr(),
                                                 ab, flags, *dims))
        rcs.append(lib.stage_grp_encoder_bwd(ones.data_ptr(), mask, ptrs(ones), ptrs(grad), grad.data_ptr(), a["T"], arena.data_ptr(), ab,
                                             flags, tmp.data_ptr(), tmp_b if tmp_bytes is None else tmp_bytes, *dims))
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((arena == 0x5A).all()) and bool((tmp == 0x5A).all()), "something was written"
        assert bool((grad == -7.0).all()), "something was written"
        return rcs

    for pooled in (0, 1):
        d = dict(dense, pooled=pooled)
        assert call(d, S=0, rows=0, cap=0) == [SHAPE] * 2
        assert call(d, L=0, rows=0, cap=0) == [SHAPE] * 2
        assert call(d, n_conv=-1) == [SHAPE] * 2
        assert call(d, n_conv=9) == [SHAPE] * 2
        assert call(d, k=4) == [SHAPE] * 2                              # what the LayerNorm -> depthwise conv kernels do not take
        assert call(d, D=20) == [SHAPE] * 2
        assert call(d, D=W) == [SHAPE] * 2                              # D > 1024
        assert call(d, rows=16, cap=16) == [SHAPE] * 2                  # rows != S * L
        assert call(d, cap=16) == [SHAPE] * 2                           # cap != rows
        r = dict(ragged, pooled=pooled)
        assert call(r, rows=0) == [SHAPE] * 2
        assert call(r, S=0) == [SHAPE] * 2
        assert call(r, cap=U - 1) == [SHAPE] * 2
        assert call(r, n_conv=0) == [SHAPE] * 2
        assert call(r, n_conv=9) == [SHAPE] * 2
        assert call(r, L=0) == [SHAPE] * 2
        assert call(r, k=4) == [SHAPE] * 2
        assert call(r, D=W) == [SHAPE] * 2
    assert call(ragged, D=64) == [SHAPE] * 2                            # pooled over ragged rows: D = 128 alone
    # a buffer one byte below what the query names: refused as such, in both directions
    for base in (dense, ragged):
        for pooled in (0, 1):
            a = dict(base, pooled=pooled)
            form = (pooled, int(a["T"] is not None))
            need = int(lib.stage_grp_encoder_arena_bytes(a["cap"], a["out_rows"] if pooled else 0, a["D"], a["n_conv"], *form))
            tneed = int(lib.stage_grp_encoder_bwd_tmp_bytes(a["cap"], a["D"], a["k"], *form))
            assert 0 < need <= big and 0 < tneed <= tmp_b
            assert call(a, arena_bytes=need - 1) == [WORKSPACE] * 2
            assert call(a, arena_bytes=need, tmp_bytes=tneed - 1, fwd=False) == [WORKSPACE]
