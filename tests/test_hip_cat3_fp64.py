"""The fused [a, b, a*b] LayerNorm-Linear kernels (csrc/cat3_fused.hip: cff_fwd_kernel<DROP, RAG>, cf_bwd_kernel MODE 0-3;
csrc/cat3_bwd_dw.hip: the eight-wave dW-inside backward), each held against a plain float64 torch restatement of

    y = ReLU(drop(LN_3D([a, b, a*b])) W^T + c)            (model/stage.py:381-385 c2q_down_projection, :276-279 concat_fc)

written HERE (``_restate``): no project kernel takes part in a reference.  The only shared pieces are the host hash of the dropout
stream (``keep_mult``, pinned bit for bit against stage_dropout_keepmask) and the host restatement of the row-info table
(``RaggedTables.rowinfo_host``, pinned row for row against stage_rag_rowinfo).  The backward kernels get random ReLU words and the
fp64 reference's mean / rstd rounded to fp32, so no forward kernel stands behind a backward test.  Through the C ABI, on the GPU.

Errors are max|got - ref| / max|ref| of a tensor ("of scale").  Bounds: 2e-5 for mean, rstd, z, y, da, db, dgamma, dbeta (what
tests/test_hip_cat3_dw.py and tests/test_hip_groups.py apply to these kernels), 4e-6 for dW, dc (test_hip_cat3_dw._check's tol_w).
Measured worst values per entry point and what the file catches (four mutated builds): docs/findings.md, finding 71.
"""
import functools

import numpy as np
import pytest
import torch

from test_hip_cat3_dw import _bits
from test_hip_dropout_parity import keep_mult

pytestmark = pytest.mark.gpu
D, K3, EPS = 128, 384, 1e-5
GUARD = 5                       # rows behind every output tensor that must keep the sentinel
SENT = -7777.25
ISENT = 0x0BADF00D
TOL, TOL_W = 2e-5, 4e-6
BAND, BAND_CAP = 1e-4, 1e-3     # |pre64| < BAND * max|pre64| carries no claim about the ReLU bit; at most BAND_CAP of the elements
# Row-by-row bound of da / db under the 2^+-24 spread of dy.  A plain fp32 torch restatement of ``_restate`` (same inputs, CPU) is
# off fp64 by at most 8.87e-7 of a ROW's own largest element (worst row of each spread case below: flat U = 4173 da 5.95e-7,
# db 7.70e-7, U = 20000 da 7.89e-7, db 7.87e-7; db of (7, 40, 15) 7.23e-7, of (300, 40, 3) 8.87e-7, of the ragged layout 8.45e-7).  The kernels split both operands of
# the product into two fp16 planes = 22 mantissa bits against fp32's 24, in two operands: they may be 2^2 * 2^2 = 16 x worse.
# (As whole tensors the same restatement is 9.2e-8 .. 4.3e-7 of scale on every gradient of these cases.)
ROW_FP32 = 8.87e-7
ROW_TOL = 16 * ROW_FP32


@pytest.fixture(autouse=True)
def _dw_on(monkeypatch):
    monkeypatch.setenv("STAGE_CAT3_DW", "1")


# ---- cases ------------------------------------------------------------------------------------------------------------
def _rag_tables(name):
    from tvqaplus_amd import ragged
    if name == "li37":                      # the layout of test_hip_cat3_dw.py: random word counts, one all-live candidate
        rng = np.random.default_rng(3)
        N, NA, Li, Lqa = 5, 5, 37, 40
        qa = np.zeros((N, NA, Lqa), bool)
        for n in range(N):
            for ai in range(NA):
                qa[n, ai, :rng.integers(0, Lqa + 1)] = True
        qa[0, 0, :] = True
        return ragged.RaggedTables(qa, rng.random((N, Li)) < 0.8, 4)
    if name == "lqa29":                     # every group has Lc <= 32: walks like MODE 1
        rng = np.random.default_rng(4)
        N, NA, Li, Lqa = 3, 5, 21, 29
        qa = np.zeros((N, NA, Lqa), bool)
        for n in range(N):
            for ai in range(NA):
                qa[n, ai, :rng.integers(0, Lqa + 1)] = True
        qa[1, 2, :] = True
        return ragged.RaggedTables(qa, rng.random((N, Li)) < 0.7, 4)
    N, NA, Lqa = 3, 5, 40
    if name == "words":                     # live word counts 0, 1, 32, 33, 40 (and others): halo 0, so Lc = the counts below
        counts = [[0, 1, 32, 33, 40], [8, 31, 39, 24, 40], [33, 0, 40, 1, 32]]
        live = np.array([[1, 1, 0, 1, 1, 1, 0, 1, 1], [1, 0, 1, 1, 0, 1, 1, 0, 0], [1, 1, 1, 1, 1, 1, 0, 0, 0]], bool)   # 7, 5, 6 live frames
        halo = 0
    else:                                   # "one_frame" / "no_frame": example 1 keeps a single live frame / none
        rng = np.random.default_rng(6)
        counts = rng.integers(1, Lqa + 1, (N, NA)).tolist()
        counts[1] = [40, 3, 33, 17, 32]
        live = rng.random((N, 6)) < 0.8
        live[1] = False
        if name == "one_frame":
            live[1, 3] = True
        else:
            assert name == "no_frame"       # RaggedTables takes it: the example gets no compact row and only its dump slot
        halo = 4
    qa = np.zeros((N, NA, Lqa), bool)
    for n in range(N):
        for ai in range(NA):
            qa[n, ai, :counts[n][ai]] = True
    return ragged.RaggedTables(qa, live, halo)


RAG_NAMES = ["li37", "lqa29", "words", "one_frame", "no_frame"]
FLAT = [(1, 1, 4096 + 77), (1, 1, 4097), (1, 1, 9000)]
MODE1 = [(31, 29, 5), (13, 32, 10), (12, 11, 32)]
MODE2 = [(7, 40, 15), (5, 40, 21), (4, 40, 26), (300, 40, 3)]
FWD_DENSE = FLAT + MODE1 + MODE2
# (case, p, spread): both DROP instantiations in every mode; dy rows over 2^+-24 on flat rows, (7, 40, 15), (300, 40, 3)
BWD_DENSE = [((1, 1, 4096 + 77), 0.1, 0), ((1, 1, 4097), 0.0, 0), ((1, 1, 9000), 0.0, 0), ((1, 1, 4096 + 77), 0.1, 24),
             ((1, 1, 20000), 0.1, 24),          # (more tiles than workgroups: the flat walk meets rows of every scale)
             ((31, 29, 5), 0.0, 0), ((13, 32, 10), 0.1, 0), ((12, 11, 32), 0.1, 0), ((7, 5, 120), 0.0, 0),
             ((7, 40, 15), 0.1, 0), ((5, 40, 21), 0.0, 0), ((4, 40, 26), 0.1, 0), ((300, 40, 3), 0.1, 0),
             ((7, 40, 15), 0.0, 24), ((300, 40, 3), 0.1, 24)]
BWD_RAG = [("li37", 0.1, 0), ("lqa29", 0.0, 0), ("words", 0.1, 0), ("one_frame", 0.0, 0), ("no_frame", 0.1, 0), ("li37", 0.1, 24)]
SEED = 4242


def _id(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=2)
def _inputs(case):
    """CPU fp32 inputs of a case (the recipe of the existing cat3 tests) and its row maps: output row r reads a[ia[r]], b[ib[r]]."""
    tab = None
    if isinstance(case, str):
        tab = _rag_tables(case)
        ri = torch.from_numpy(tab.rowinfo_host().astype(np.int64))
        U, a_rows, b_rows, ia, ib = tab.U, tab.N * tab.NA * tab.Lqa, tab.Fc, ri[:, 0].contiguous(), ri[:, 1].contiguous()
        rep = inner = 1
        seed = 100 + RAG_NAMES.index(case)
    else:
        rep, inner, G = case
        U = G * rep * inner if rep > 1 else G
        r = torch.arange(U)
        a_rows, b_rows, ib = U // rep, U, r
        ia = (r // (rep * inner)) * inner + r % inner if rep > 1 else r
        seed = 11 + rep + 1000 * inner
    g = torch.Generator().manual_seed(seed)
    return dict(tab=tab, U=U, rep=rep, inner=inner, ia=ia, ib=ib, a=torch.randn(a_rows, D, generator=g), b=torch.randn(b_rows, D, generator=g),
                gamma=1 + 0.1 * torch.randn(K3, generator=g), beta=0.1 * torch.randn(K3, generator=g),
                W=0.08 * torch.randn(D, K3, generator=g), c=0.1 * torch.randn(D, generator=g))


def _keep(p, U):
    """(U, 3D) multipliers of dropout stream SEED: element index row * 3D + col, `row` the (compact) output row"""
    return keep_mult(SEED, p, U * K3).view(U, K3) if p > 0 else torch.ones(U, K3)


def _restate(inp, keep, dt, dyg=None):
    """the reference: plain torch in dtype ``dt``.  dyg = dy * gate: returns the gradients of (pre * dyg).sum() as well."""
    a, b, gamma, beta, W, c = (inp[k].to(dt).requires_grad_(dyg is not None) for k in ("a", "b", "gamma", "beta", "W", "c"))
    A, B = a[inp["ia"]], b[inp["ib"]]
    x = torch.cat([A, B, A * B], -1)
    mu = x.mean(-1, keepdim=True)
    rstd = (((x - mu) ** 2).mean(-1, keepdim=True) + EPS) ** -0.5
    z = ((x - mu) * rstd * gamma + beta) * keep.to(dt)
    pre = z @ W.t() + c
    out = dict(mean=mu.detach().squeeze(1), rstd=rstd.detach().squeeze(1), z=z.detach(), pre=pre.detach())
    if dyg is not None:
        (pre * dyg.to(dt)).sum().backward()
        out.update(da=a.grad, db=b.grad, dgamma=gamma.grad, dbeta=beta.grad, dW=W.grad, dc=c.grad)
    return out


@functools.lru_cache(maxsize=2)
def _fwd_ref(case, p):
    inp = _inputs(case)
    keep = _keep(p, inp["U"])
    ref = _restate(inp, keep, torch.float64)
    ref["keep"] = keep
    return ref


def _bwd_problem(case, p, spread):
    inp = _inputs(case)
    U = inp["U"]
    g = torch.Generator().manual_seed(7 + spread)
    dy = torch.randn(U, D, generator=g)
    if spread:                              # random order: small rows follow large ones inside every workgroup's share
        dy = dy * torch.exp2(torch.randint(-spread, spread + 1, (U, 1), generator=g).float())
    mask = torch.randint(-2 ** 31, 2 ** 31 - 1, (D // 32, U), generator=g, dtype=torch.int64).to(torch.int32)
    return inp, dy, mask, dy.double() * _bits(mask, U).double()


@functools.lru_cache(maxsize=2)
def _bwd_ref(case, p, spread):
    inp, dy, mask, dyg = _bwd_problem(case, p, spread)
    ref = _restate(inp, _keep(p, inp["U"]), torch.float64, dyg)
    del ref["z"], ref["pre"]
    ref.update(dy=dy, mask=mask, mean32=ref["mean"].float(), rstd32=ref["rstd"].float())
    return ref


# ---- helpers ----------------------------------------------------------------------------------------------------------
def _scale_err(got, ref):
    ref = ref.double()
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    s = float(ref.abs().max())
    assert s > 0
    return float((got - ref).abs().max()) / s


def _row_err(got, ref):
    """worst row of max_c |got - ref| / max_c |ref| over the rows with a non-zero reference"""
    ref = ref.double()
    got = got.detach().double().cpu()
    s = ref.abs().amax(1)
    sel = s > 0
    assert bool(sel.any())
    return float(((got - ref).abs().amax(1)[sel] / s[sel]).max())


class _Out:
    """a device tensor of ``rows`` rows with GUARD sentinel rows behind it"""

    def __init__(self, rows, cols, fill, dtype=torch.float32):
        self.rows, self.sent = rows, (ISENT if dtype == torch.int32 else SENT)
        self.buf = torch.full((rows + GUARD, cols) if cols else (rows + GUARD,), fill, dtype=dtype, device="cuda")
        self.buf[rows:] = self.sent
        self.t = self.buf[:rows]

    def ptr(self):
        return self.buf.data_ptr()

    def guard_ok(self):
        return bool((self.buf[self.rows:] == self.sent).all())


def _dev(inp, *names):
    return [inp[k].cuda().contiguous() for k in names]


def _layout(case, dev):
    from tvqaplus_amd import ragged
    lay = ragged.RaggedLayout(_inputs(case)["tab"], dev)
    assert torch.equal(lay.rowinfo.cpu().view(-1, 4)[:lay.U], torch.from_numpy(_inputs(case)["tab"].rowinfo_host()))
    return lay


# ---- forward ------------------------------------------------------------------------------------------------------------
def _run_fwd(lib, case, inp, dv, p, lay, fill, ws_fill):
    from tvqaplus_amd import _lib
    U = inp["U"]
    a, b, gamma, beta, W, c = dv
    z, y = _Out(U, K3, fill), _Out(U, D, fill)
    mean, rstd = _Out(U, 0, fill), _Out(U, 0, fill)
    mask = _Out(D // 32 * U, 0, 0x55555555 if fill != fill else 0, torch.int32)          # [D/32][rows] words, GUARD words behind
    wsb = lib.stage_cat3_ln_gemm_fwd_ws_bytes()
    ws = torch.full((wsb,), ws_fill, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    if lay is None:
        assert lib.stage_cat3_ln_gemm_fwd_supported(U, D, inp["rep"], inp["inner"])
        _lib.check(lib.stage_cat3_ln_gemm_fwd(a.data_ptr(), b.data_ptr(), gamma.data_ptr(), beta.data_ptr(), W.data_ptr(), c.data_ptr(),
                                              z.ptr(), mean.ptr(), rstd.ptr(), y.ptr(), mask.ptr(), U, D, inp["rep"], inp["inner"], EPS, p,
                                              SEED, ws.data_ptr(), wsb, st), "fused fwd")
    else:
        assert lib.stage_cat3_ln_gemm_fwd_rag_supported(U, a.shape[0], b.shape[0], D)
        _lib.check(lib.stage_cat3_ln_gemm_fwd_rag(a.data_ptr(), b.data_ptr(), gamma.data_ptr(), beta.data_ptr(), W.data_ptr(), c.data_ptr(),
                                                  z.ptr(), mean.ptr(), rstd.ptr(), y.ptr(), mask.ptr(), lay.rowinfo.data_ptr(), U, a.shape[0],
                                                  b.shape[0], D, EPS, p, SEED, ws.data_ptr(), wsb, st), "fused fwd rag")
    torch.cuda.synchronize()
    return dict(z=z, mean=mean, rstd=rstd, y=y, mask=mask)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("case", FWD_DENSE + RAG_NAMES, ids=_id)
def test_fused_forward_against_fp64(hip_device, case, p):
    """stage_cat3_ln_gemm_fwd / _rag with z stored: mean, rstd, z, y of scale 2e-5 off fp64; z == 0 exactly where the host hash drops;
    ReLU words == (y > 0) exactly and == (pre64 > 0) outside the band; guard rows; a second call into NaN outputs over a 0xFF
    workspace gives the same bits."""
    from tvqaplus_amd import _lib
    lib = _lib.load()
    inp, ref = _inputs(case), _fwd_ref(case, p)
    U = inp["U"]
    lay = _layout(case, hip_device) if inp["tab"] is not None else None
    dv = _dev(inp, "a", "b", "gamma", "beta", "W", "c")
    o1 = _run_fwd(lib, case, inp, dv, p, lay, 0.0, 0)
    o2 = _run_fwd(lib, case, inp, dv, p, lay, float("nan"), 0xFF)
    for k in o1:
        assert o1[k].guard_ok() and o2[k].guard_ok(), k
        assert torch.equal(o1[k].t, o2[k].t), k
    y = o1["y"].t
    errs = {k: _scale_err(o1[k].t, ref[k]) for k in ("mean", "rstd", "z")}
    errs["y"] = _scale_err(y, ref["pre"].clamp(min=0))
    print("fwd %-14s p %.1f: " % (_id(case), p) + "  ".join("%s %.2e" % kv for kv in errs.items()))
    for k in o1:
        assert k == "mask" or torch.isfinite(o1[k].t).all(), k
    for k, e in errs.items():
        assert e <= TOL, (k, e)
    assert torch.equal(o1["z"].t.cpu() == 0, ref["keep"] == 0)
    bits = _bits(o1["mask"].t.view(D // 32, U), U)
    assert torch.equal(bits, y > 0)
    pre = ref["pre"]
    claim = pre.abs() >= BAND * pre.abs().max()
    share = 1.0 - float(claim.double().mean())
    assert share <= BAND_CAP, share                 # (the reference alone: 0.034 - 0.046 % on these inputs)
    assert torch.equal(bits.cpu()[claim], (pre > 0)[claim])


def test_forward_declines_groups_shorter_than_a_tile(hip_device):
    """cff_fwd_kernel finds the row of a broadcast `a` with ONE group step per 32-row tile: rep * inner < 32 (a tile over three groups)
    would read the wrong rows of `a`.  The entry point declines before anything is launched; outputs stay untouched."""
    from tvqaplus_amd import _lib
    lib = _lib.load()
    for rep, inner, G in ((2, 11, 187), (2, 15, 137)):
        U = G * rep * inner
        assert U >= 4096 and not lib.stage_cat3_ln_gemm_fwd_supported(U, D, rep, inner)
    assert lib.stage_cat3_ln_gemm_fwd_supported(4096, D, 2, 16) and lib.stage_cat3_ln_gemm_fwd_supported(12 * 11 * 32, D, 12, 11)
    rep, inner, G = 2, 11, 187
    U = G * rep * inner
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(G * inner, D, generator=g).cuda(), torch.randn(U, D, generator=g).cuda()
    gamma, beta, W, c = torch.ones(K3).cuda(), torch.zeros(K3).cuda(), torch.randn(D, K3, generator=g).cuda(), torch.zeros(D).cuda()
    outs = [_Out(U, K3, SENT), _Out(U, 0, SENT), _Out(U, 0, SENT), _Out(U, D, SENT), _Out(D // 32 * U, 0, ISENT, torch.int32)]
    wsb = lib.stage_cat3_ln_gemm_fwd_ws_bytes()
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    code = lib.stage_cat3_ln_gemm_fwd(a.data_ptr(), b.data_ptr(), gamma.data_ptr(), beta.data_ptr(), W.data_ptr(), c.data_ptr(),
                                      *[o.ptr() for o in outs], U, D, rep, inner, EPS, 0.0, SEED, ws.data_ptr(), wsb,
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert code == _lib.STAGE_ERR_SHAPE
    for o in outs:
        assert bool((o.buf == o.sent).all())


# ---- backward -----------------------------------------------------------------------------------------------------------
GRADS = ("da", "db", "dgamma", "dbeta", "dW", "dc")


def _run_bwd(lib, entry, inp, dv, ref_dev, p, lay, fill, ws_fill, alias=False):
    """one call of a backward entry point into fresh guarded outputs (da, db[_fc], dgamma, dbeta[, dW, dc])"""
    from tvqaplus_amd import _lib
    U = inp["U"]
    a, b, gamma, beta, W = dv
    dy, mask, mean, rstd = ref_dev
    o = dict(da=_Out(a.shape[0], D, fill), db=_Out(b.shape[0], D, fill), dgamma=_Out(K3, 0, fill), dbeta=_Out(K3, 0, fill))
    if alias:                               # db_fc IS b_fc (include/stage_hip.h allows it): the kernel reads a row before it writes it
        o["db"].t.copy_(b)
        b = o["db"].t
    dw = entry == "dw"
    if dw:
        o.update(dW=_Out(D, K3, fill), dc=_Out(D, 0, fill))
    st = torch.cuda.current_stream().cuda_stream
    head = (dy.data_ptr(), mask.data_ptr(), W.data_ptr(), a.data_ptr(), b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr())
    grads = tuple(o[k].ptr() for k in GRADS if k in o)
    if lay is None:
        rep, inner = inp["rep"], inp["inner"]
        wsb = (lib.stage_cat3_bwd_dw_ws_bytes if dw else lib.stage_cat3_dx_ln_bwd_ws_bytes)(U, D, rep, inner)
        ws = torch.full((wsb,), ws_fill, dtype=torch.uint8, device="cuda")
        tail = (U, D, rep, inner, p, SEED, ws.data_ptr(), wsb, st)
        if dw:
            _lib.check(lib.stage_cat3_bwd_dw(*head, beta.data_ptr(), *grads, *tail), "dW-inside bwd")
        else:
            _lib.check(lib.stage_cat3_dx_ln_bwd(*head, *grads, *tail), "fused bwd")
    else:
        G = lay.N * lay.NA
        wsb = lib.stage_cat3_bwd_dw_rag_ws_bytes(G, lay.Lqa) if dw else lib.stage_cat3_dx_ln_bwd_rag_ws_bytes(G, lay.Li, lay.Lqa)
        ws = torch.full((wsb,), ws_fill, dtype=torch.uint8, device="cuda")
        wtab = None if entry == "dx_chunks" else lay.wtab.data_ptr()
        tail = (lay.gdesc.data_ptr(), wtab, U, lay.Fc, D, G, lay.Li, lay.Lqa, p, SEED, ws.data_ptr(), wsb, st)
        if dw:
            _lib.check(lib.stage_cat3_bwd_dw_rag(*head, beta.data_ptr(), *grads, *tail), "dW-inside rag bwd")
        else:
            _lib.check(lib.stage_cat3_dx_ln_bwd_rag(*head, *grads, *tail), "fused rag bwd")
    torch.cuda.synchronize()
    return o


def _check_bwd(tag, o, ref, spread, rows_da=True, owned=None):
    errs = {}
    for k in GRADS:
        if k not in o:
            continue
        got, exp = o[k].t, ref[k]
        if k == "db" and owned is not None:
            got, exp = got[owned.cuda()], exp[owned]
        assert torch.isfinite(got).all(), k
        errs[k] = _scale_err(got, exp)
    rows = {}
    if spread:
        rows["db"] = _row_err(o["db"].t if owned is None else o["db"].t[owned.cuda()], ref["db"] if owned is None else ref["db"][owned])
        if rows_da:
            rows["da"] = _row_err(o["da"].t, ref["da"])
    print("bwd %s: " % tag + "  ".join("%s %.2e" % kv for kv in errs.items()) + "".join("  row-%s %.2e" % kv for kv in rows.items()))
    for k, e in errs.items():
        assert e <= (TOL_W if k in ("dW", "dc") else TOL), (k, e)
    for k, e in rows.items():
        assert e <= ROW_TOL, ("row by row", k, e)


def _bwd_common(lib, entry, case, p, spread, lay):
    inp, ref = _inputs(case), _bwd_ref(case, p, spread)
    dv = _dev(inp, "a", "b", "gamma", "beta", "W")
    ref_dev = [ref[k].cuda() for k in ("dy", "mask", "mean32", "rstd32")]
    o1 = _run_bwd(lib, entry, inp, dv, ref_dev, p, lay, SENT, 0)
    o2 = _run_bwd(lib, entry, inp, dv, ref_dev, p, lay, float("nan"), 0xFF)
    return inp, ref, dv, ref_dev, o1, o2


@pytest.mark.parametrize("entry", ["dx", "dw"])
@pytest.mark.parametrize("case,p,spread", BWD_DENSE, ids=_id)
def test_dense_backward_against_fp64(hip_device, case, p, spread, entry):
    """stage_cat3_dx_ln_bwd (cf_bwd_kernel MODE 0 / 1 / 2) and stage_cat3_bwd_dw on flat and broadcast rows"""
    from tvqaplus_amd import _lib
    lib = _lib.load()
    rep, inner, G = case
    U = _inputs(case)["U"]
    if not (lib.stage_cat3_bwd_dw_supported if entry == "dw" else lib.stage_cat3_dx_ln_bwd_supported)(U, D, rep, inner):
        pytest.skip("fused backward switched off")
    inp, ref, _, _, o1, o2 = _bwd_common(lib, entry, case, p, spread, None)
    for k in o1:
        assert o1[k].guard_ok() and o2[k].guard_ok(), k
        assert torch.equal(o1[k].t, o2[k].t), k
    _check_bwd("%s %-12s p %.1f spread %2d" % (entry, _id(case), p, spread), o1, ref, spread, rows_da=rep == 1)


@pytest.mark.parametrize("entry", ["dx_chunks", "dx_table", "dw"])
@pytest.mark.parametrize("case,p,spread", BWD_RAG, ids=_id)
def test_ragged_backward_against_fp64(hip_device, case, p, spread, entry):
    """stage_cat3_dx_ln_bwd_rag without (one workgroup per (group, chunk)) and with the balanced work table, stage_cat3_bwd_dw_rag:
    db_fc rows that no compact row owns keep what they held, da rows of words at or behind a group's Lc are the reference's zeros"""
    from tvqaplus_amd import _lib
    lib = _lib.load()
    lay = _layout(case, hip_device)
    G = lay.N * lay.NA
    if not (lib.stage_cat3_bwd_dw_rag_supported if entry == "dw" else lib.stage_cat3_dx_ln_bwd_rag_supported)(lay.U, lay.Fc, D, G, lay.Li, lay.Lqa):
        pytest.skip("fused backward switched off")
    assert lay.wtab is not None and lay.n_wg == lib.stage_cat3_rag_work_groups() == lib.stage_cat3_bwd_dw_rag_work_groups()
    inp, ref, _, _, o1, o2 = _bwd_common(lib, entry, case, p, spread, lay)
    owned = torch.zeros(lay.Fc, dtype=torch.bool)
    owned[inp["ib"]] = True
    assert int(owned.sum()) == lay.U and not bool(owned.all())         # one compact row per owned row; every layout has dump slots
    dead = torch.ones(G * lay.Lqa, dtype=torch.bool)
    dead[inp["ia"]] = False
    assert bool(dead.any()) and not bool(ref["da"][dead].any())
    for k in o1:
        assert o1[k].guard_ok() and o2[k].guard_ok(), k
        if k == "db":
            assert torch.equal(o1[k].t[owned.cuda()], o2[k].t[owned.cuda()])
            assert bool((o1[k].t[~owned.cuda()] == SENT).all()) and bool(torch.isnan(o2[k].t[~owned.cuda()]).all())
        else:
            assert torch.equal(o1[k].t, o2[k].t), k
    _check_bwd("%s %-10s p %.1f spread %2d" % (entry, case, p, spread), o1, ref, spread, rows_da=False, owned=owned)
    assert not bool(o1["da"].t[dead.cuda()].any())


@pytest.mark.parametrize("entry", ["dx_table", "dw"])
def test_ragged_backward_with_db_aliased_to_b(hip_device, entry):
    """db_fc == b_fc (the product's attention group does this): the same bits as into a separate db_fc, b's values elsewhere"""
    from tvqaplus_amd import _lib
    lib = _lib.load()
    case, p = "li37", 0.1
    lay = _layout(case, hip_device)
    G = lay.N * lay.NA
    if not (lib.stage_cat3_bwd_dw_rag_supported if entry == "dw" else lib.stage_cat3_dx_ln_bwd_rag_supported)(lay.U, lay.Fc, D, G, lay.Li, lay.Lqa):
        pytest.skip("fused backward switched off")
    inp, ref, dv, ref_dev, o1, _ = _bwd_common(lib, entry, case, p, 0, lay)
    oa = _run_bwd(lib, entry, inp, dv, ref_dev, p, lay, SENT, 0, alias=True)
    owned = torch.zeros(lay.Fc, dtype=torch.bool)
    owned[inp["ib"]] = True
    owned = owned.cuda()
    for k in o1:
        assert oa[k].guard_ok(), k
        if k == "db":
            assert torch.equal(o1[k].t[owned], oa[k].t[owned])
            assert torch.equal(oa[k].t[~owned], dv[1][~owned])
        else:
            assert torch.equal(o1[k].t, oa[k].t), k
