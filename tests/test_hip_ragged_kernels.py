"""-m gpu: the ragged-row kernels one by one, through the C ABI, against plain fp64 evaluations of the same operations.

What runs on ragged rows (tvqaplus_amd/ragged.py, docs/ragged.md) and was only ever reached through whole-model tests:

* csrc/ragged.hip       stage_rag_rowinfo, stage_rag_ctx_rows, stage_rag_fill_pooled       -- exact, against the host restatements
* csrc/rowops.hip       stage_layernorm_gather_fwd/bwd, stage_l2norm_gather_fwd           -- fp64 on the gathered rows
* csrc/ln_dwconv.hip    stage_ln_dwconv_rag_fwd/bwd                                       -- fp64, each sequence alone
* csrc/rowops.hip       stage_ln_masked_max_rag_fwd/bwd                                   -- fp64, each sequence alone, first maximum wins
* csrc/groups.hip       stage_grp_encoder_fwd/bwd with tables (groups.encoder_block_rag)  -- oracle.encoder_block in fp64, each sequence alone

The reference of every ``seq`` table cuts the rows [start, start + len) of a sequence out and evaluates plain torch in float64 on them
(F.layer_norm, F.conv1d with zero padding at the sequence's OWN ends, oracle.mask_logits, oracle.encoder_block), so a halo row read
across a sequence boundary, a position table indexed by the compact row, a dropout counter that is not the compact row, a dropped
partial of a weight gradient or a wrong statistic behind a chunk edge are all errors of order one.  With dropout the reference carries
the host restatement of the keep stream (tests/test_hip_dropout_parity.py: keep_mult, pinned to stage_dropout_keepmask), counter = compact row.

Tolerance: the per-kernel bound of tests/test_hip_ops.py, 2e-4 under conftest.rel_err, gradients included.  Integer tables and the
-1e10 fills compare exactly.  Masked max: the first maximum wins (torch.argmax); a (group, column) whose two largest fp64 values lie
within 1e-4 of each other may be routed to the other row by an fp32 kernel, so its upstream gradient is set to 0 and its arg-max is
not compared -- at most 1 % of the pairs may be treated so.

Measured on an MI355X (worst rel_err of each test over its cases; bound 2e-4): tables exact; gathered LayerNorm 2.9e-6 (d gamma, K 300),
l2norm 3.3e-8; ln_dwconv_rag 1.5e-5 (db over 14 727 rows; h 8.5e-7, dx 5.5e-7); ln_masked_max_rag 1.1e-6 (d gamma; out and dx 1.5e-7),
near ties 0.023 % of 8 576 pairs; pooled encoder group 7.6e-6, unpooled 1.4e-5 (both: the pointwise conv's weight gradient) -- the
oracle's own fp32 evaluation on the CPU is off fp64 by 5.8e-6 / 1.1e-5 there, so the group needs no bound of its own.  The file runs in 5 s.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from oracle import stage_oracle as O
from test_hip_dropout_parity import keep_mult

pytestmark = pytest.mark.gpu

TOL = 2e-4              # tests/test_hip_ops.py: every kernel, outputs and gradients
EPS = 1e-5
NEG = -1e10
NEG32 = float(np.float32(NEG))
TIE_GAP = 1e-4          # fp64 top-two gap below which an fp32 arg-max may differ
SENT = -7777.0          # what output rows that no sequence owns must still hold after a call
ISENT = -77777
GUARD = 5               # rows behind the last one a table kernel may write
KEY = "enc"


@pytest.fixture(scope="module")
def lib(hip_device):
    from tvqaplus_amd import _lib
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    from tvqaplus_amd import _lib
    _lib.check(rc, what)


def _p(t):
    return None if t is None else t.data_ptr()


def _hold(name, got, ref, tol=TOL):
    """finite, and within tol of the fp64 reference; prints the figure (run with -s to collect them)"""
    assert bool(torch.isfinite(got).all()), (name, "not finite: a row of another sequence / a gap row was read, or an element not written")
    e = rel_err(got, ref)
    print("    %-28s rel_err %.3e" % (name, e))
    assert e < tol, (name, e, tol)
    return e


# =====================================================================================================================
# 1. index tables, exact
# =====================================================================================================================
def _statement_masks(N, NA, Li, Lqa, seed):
    """QA word masks with: a statement without a valid word, a full one, one with holes; an example without a live frame, one with all live"""
    rng = np.random.default_rng(seed)
    qa = np.zeros((N, NA, Lqa), bool)
    for n in range(N):
        for a in range(NA):
            qa[n, a, :rng.integers(1, Lqa + 1)] = True
    qa[0, 0, :] = False
    qa[0, 1, :] = True
    qa[0, 2, :] = False
    qa[0, 2, [0, 2, 3, Lqa // 2]] = True
    fl = rng.random((N, Li)) < 0.7
    fl[0, 0] = True
    fl[1, :] = False
    fl[2, :] = True
    return qa, fl


def test_rowinfo_on_the_device_equals_the_host_restatement(hip_device, lib):
    from tvqaplus_amd import ragged
    N, NA, Li, Lqa = 3, 5, 7, 13
    qa, fl = _statement_masks(N, NA, Li, Lqa, 1)
    tab = ragged.RaggedTables(qa, fl, 4)
    lay = ragged.RaggedLayout(tab, hip_device)
    U, S = tab.U, tab.S
    assert S * Lqa > 256 and (S * Lqa) % 256 != 0            # more than one block, the last one partly filled
    assert (tab.Lc == 0).any() and (tab.Lc == Lqa).any() and (tab.Lc[tab.Lc > 0] < Lqa).any()
    out = torch.full((U + GUARD, 4), ISENT, dtype=torch.int32, device=hip_device)
    _ok(lib.stage_rag_rowinfo(lay.seq.data_ptr(), lay.seqfc.data_ptr(), S, Lqa, out.data_ptr(), _st()), "stage_rag_rowinfo")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ref = tab.rowinfo_host()
    assert ref.shape == (U, 4)
    assert np.array_equal(got[:U], ref)                          # every row below U written, with the host's numbers
    assert (got[U:] == ISENT).all()                              # nothing behind
    assert np.array_equal(lay.rowinfo.view(-1, 4)[:U].cpu().numpy(), ref)      # the table the product's layout object built


@pytest.mark.parametrize("L", [50, 300])
def test_ctx_rows_on_the_device_equal_the_host_restatement(hip_device, lib, L):
    from tvqaplus_amd import ragged
    N, Li, halo = 2, 9, 6
    rng = np.random.default_rng(L)
    lens = rng.integers(0, L + 1, size=(N, Li))
    lens.reshape(-1)[:5] = [0, 1, L - 6, L - 5, L]               # no row; one word; len + halo == L; one past; the whole frame
    lens[1, Li - 1] = 0
    tab = ragged.CtxTables(lens, L, halo)
    lay = ragged.CtxLayout(tab, hip_device)
    U = tab.U
    out = torch.full((U + GUARD,), ISENT, dtype=torch.int32, device=hip_device)
    _ok(lib.stage_rag_ctx_rows(lay.cq.data_ptr(), N * Li, L, out.data_ptr(), _st()), "stage_rag_ctx_rows")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ref = tab.src_rows_host()
    assert np.array_equal(got[:U], ref)
    assert (got[U:] == ISENT).all()
    assert np.array_equal(lay.src_rows[:U].cpu().numpy(), ref)


def test_fill_pooled_writes_its_rows_and_nothing_else(hip_device, lib):
    rows, D = 37, 128
    out = torch.full((rows + GUARD, D), SENT, device=hip_device)
    idx = torch.full((rows + GUARD, D), ISENT, dtype=torch.int32, device=hip_device)
    _ok(lib.stage_rag_fill_pooled(out.data_ptr(), idx.data_ptr(), rows, D, _st()), "stage_rag_fill_pooled")
    torch.cuda.synchronize()
    assert bool((out[:rows] == NEG32).all()) and bool((idx[:rows] == 0).all())
    assert bool((out[rows:] == SENT).all()) and bool((idx[rows:] == ISENT).all())


# =====================================================================================================================
# 2. gathered LayerNorm / l2norm: the first kernels of the input MLP on a ragged context stream
# =====================================================================================================================
def _ctx_gather(dev, K, seed):
    """the gather table of a CtxLayout (11 frames of 20 positions) and a padded feature tensor whose unread rows are NaN"""
    from tvqaplus_amd import ragged
    L = 20
    lens = np.array([[0, L, 5, 1, 17, 18, 0, L, 9, 12, 3]])
    tab = ragged.CtxTables(lens, L, 3)
    lay = ragged.CtxLayout(tab, dev)
    src = torch.from_numpy(tab.src_rows_host().astype(np.int64))
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(lens.size * L, K, generator=g) * 2.0 + 0.25
    read = torch.zeros(x.shape[0], dtype=torch.bool)
    read[src] = True
    assert 0 < int(read.sum()) == tab.U < x.shape[0]
    return lay, src, x, read


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("K", [768, 300, 48])
def test_layernorm_gather_vs_fp64(hip_device, lib, K, p):
    dev = hip_device
    lay, src, x, read = _ctx_gather(dev, K, 7 * K)
    U, seed = lay.U, 0x1234ABCD77
    g = torch.Generator().manual_seed(K)
    gamma = 1.0 + 0.2 * torch.randn(K, generator=g)
    beta = 0.2 * torch.randn(K, generator=g)
    dy = torch.randn(U, K, generator=g)
    xp = x.clone()
    xp[~read] = float("nan")
    xd, gd, bd, dyd = xp.to(dev), gamma.to(dev), beta.to(dev), dy.to(dev)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    y, mean, rstd, dgam, dbet = nan(U, K), nan(U), nan(U), nan(K), nan(K)
    _ok(lib.stage_layernorm_gather_fwd(xd.data_ptr(), lay.src_rows.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                       rstd.data_ptr(), U, K, EPS, p, seed, _st()), "stage_layernorm_gather_fwd")
    wsb = lib.stage_ln_bwd_ws_bytes(K)
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=dev)
    _ok(lib.stage_layernorm_gather_bwd(dyd.data_ptr(), xd.data_ptr(), lay.src_rows.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gd.data_ptr(),
                                       dgam.data_ptr(), dbet.data_ptr(), U, K, p, seed, ws.data_ptr(), wsb, _st()), "stage_layernorm_gather_bwd")
    torch.cuda.synchronize()
    m = keep_mult(seed, p, U * K).view(U, K).double() if p > 0 else torch.ones(U, K, dtype=torch.float64)
    v = x.double()[src]
    mu = v.mean(-1)
    rs = 1.0 / torch.sqrt(v.var(-1, unbiased=False) + EPS)
    xh = (v - mu[:, None]) * rs[:, None]
    dym = dy.double() * m
    _hold("y", y, F.layer_norm(v, (K,), gamma.double(), beta.double(), EPS) * m)
    _hold("mean", mean, mu)
    _hold("rstd", rstd, rs)
    _hold("dgamma", dgam, (dym * xh).sum(0))
    _hold("dbeta", dbet, dym.sum(0))
    if p > 0:
        assert torch.equal((y == 0).cpu(), m == 0)              # the dropped elements are the ones the stream names for the COMPACT row


@pytest.mark.parametrize("K", [768, 300, 48])
def test_l2norm_gather_vs_fp64(hip_device, lib, K):
    dev = hip_device
    lay, src, x, read = _ctx_gather(dev, K, 11 * K)
    U = lay.U
    x[src[U // 2]] = 0.0                                         # an all-zero feature row: x / max(|x|, eps) = 0 (eps as tests/test_hip_feat16.py)
    xp = x.clone()
    xp[~read] = float("nan")
    xd = xp.to(dev)
    y = torch.full((U, K), float("nan"), device=dev)
    _ok(lib.stage_l2norm_gather_fwd(xd.data_ptr(), lay.src_rows.data_ptr(), y.data_ptr(), U, K, 1e-12, _st()), "stage_l2norm_gather_fwd")
    torch.cuda.synchronize()
    _hold("xn", y, F.normalize(x.double()[src], dim=-1, eps=1e-12))
    assert bool((y[U // 2] == 0).all())


# =====================================================================================================================
# 3. LayerNorm (+ residual / position table, + dropout) -> depthwise conv on ragged sequences
# =====================================================================================================================
def _lengths(case):
    rng = np.random.default_rng(17)
    if case == "short":
        return [1, 2, 3, 1, 7, 4, 5, 6]
    if case == "cls":
        l = rng.integers(1, 41, size=37)
        l[5] = 40
        l[11] = 1
        return [int(v) for v in l]
    if case == "chunks":
        return [1, 43, 44, 45, 87, 88, 89, 130, 2, 61, 44, 130]
    if case == "nores":
        l = rng.integers(1, 10, size=12)
        l[0], l[7] = 9, 1
        return [int(v) for v in l]
    if case == "taps":
        return list(range(1, 13))
    if case == "capped":
        return [int(v) for v in rng.integers(1, 7, size=4200)]
    raise KeyError(case)


LD_CASES = [
    # lengths   Lmax  D   k  residual  p    gaps
    ("short",   7,   16,  7, "pe",   0.0, False),     # window wider than the sequence, length 1
    ("cls",     40,  128, 5, "res",  0.1, True),      # the classifier encoder's shape
    ("chunks",  130, 128, 7, "pe",   0.1, True),      # three chunks of 44: sequences ending on / before / behind a chunk edge
    ("nores",   9,   64,  3, None,   0.0, False),     # res == NULL, sum_out == NULL
    ("taps",    12,  32,  1, "pe",   0.0, False),     # the outer tap counts
    ("taps",    12,  32,  9, "pe",   0.0, False),
    ("capped",  6,   128, 5, "res",  0.0, False),     # 4200 items > 512 * 256 / (D / 4) = 4096: grid-capped backward, accumulators carry across items
]


def _by_length(seq):
    """{length: (M, length) int64 row indices} -- sequences of one length as a batch; batch entries do not interact"""
    out = {}
    for s, l in seq:
        out.setdefault(l, []).append(torch.arange(s, s + l))
    return {l: torch.stack(v) for l, v in out.items()}


@pytest.mark.parametrize("case,Lmax,D,k,resmode,p,gaps", LD_CASES, ids=["%s-k%d" % (c[0], c[3]) for c in LD_CASES])
def test_ln_dwconv_rag_vs_fp64(hip_device, lib, case, Lmax, D, k, resmode, p, gaps):
    from tvqaplus_amd import _lib
    dev = hip_device
    lens = _lengths(case)
    assert max(lens) == Lmax and min(lens) == 1
    rng = np.random.default_rng(3)
    g = torch.Generator().manual_seed(1000 + D + k)
    seq, row = [], 0
    for l in lens:
        if gaps:
            row += int(rng.integers(1, 4))
        seq.append((row, l))
        row += l
    R = row + (2 if gaps else 0)
    S = len(seq)
    live = torch.zeros(R, dtype=torch.bool)
    for s, l in seq:
        live[s:s + l] = True
    gap = ~live
    assert bool(gap.any()) == gaps
    live_d, gap_d = live.to(dev), gap.to(dev)
    seqt = torch.tensor([[s, l, 0, 0] for s, l in seq], dtype=torch.int32).to(dev)
    seed = 0xABCDEF0123 + k

    x, res, dh, dxa = (torch.randn(R, D, generator=g) for _ in range(4))
    pe = torch.randn(Lmax, D, generator=g)
    gamma, beta = 1.0 + 0.2 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
    w, b = 0.5 * torch.randn(D, 1, k, generator=g), 0.2 * torch.randn(D, generator=g)

    def poisoned(t):                                             # an input: NaN in the rows between the sequences
        t = t.clone()
        t[gap] = float("nan")
        return t.to(dev)
    xd, dhd, dxad = poisoned(x), poisoned(dh), poisoned(dxa)
    resd = poisoned(res) if resmode == "res" else None
    ped = pe.to(dev) if resmode == "pe" else None
    gd, bd, wd, cd = gamma.to(dev), beta.to(dev), w.to(dev), b.to(dev)
    sent = lambda *s: torch.full(s, SENT, device=dev)
    h, mean, rstd = sent(R, D), sent(R), sent(R)
    sum_out = sent(R, D) if resmode else None

    if resmode == "pe":                                          # pe and res together: refused before a launch
        rc = lib.stage_ln_dwconv_rag_fwd(xd.data_ptr(), xd.data_ptr(), ped.data_ptr(), sum_out.data_ptr(), gd.data_ptr(), bd.data_ptr(), wd.data_ptr(),
                                         cd.data_ptr(), h.data_ptr(), mean.data_ptr(), rstd.data_ptr(), seqt.data_ptr(), S, Lmax, D, k, EPS, p, seed, _st())
        assert rc == _lib.STAGE_ERR_SHAPE
        torch.cuda.synchronize()
        assert bool((h == SENT).all())
    _ok(lib.stage_ln_dwconv_rag_fwd(xd.data_ptr(), _p(resd), _p(ped), _p(sum_out), gd.data_ptr(), bd.data_ptr(), wd.data_ptr(), cd.data_ptr(),
                                    h.data_ptr(), mean.data_ptr(), rstd.data_ptr(), seqt.data_ptr(), S, Lmax, D, k, EPS, p, seed, _st()),
        "stage_ln_dwconv_rag_fwd")
    torch.cuda.synchronize()

    # ---- fp64, each sequence alone -------------------------------------------------------------------------------
    m = keep_mult(seed, p, R * D).view(R, D).double() if p > 0 else torch.ones(R, D, dtype=torch.float64)     # counter: the compact row
    P64 = [t.double().requires_grad_(True) for t in (gamma, beta, w, b)]
    v_all = x.double()
    if resmode == "res":
        v_all = v_all + res.double()
    h_ref, s_ref = torch.zeros(R, D, dtype=torch.float64), torch.zeros(R, D, dtype=torch.float64)
    mu_ref, rs_ref, dv_ref = torch.zeros(R, dtype=torch.float64), torch.zeros(R, dtype=torch.float64), torch.zeros(R, D, dtype=torch.float64)
    total, leaves = 0.0, []
    for l, rows in _by_length(seq).items():
        v = v_all[rows]                                          # (M, l, D)
        if resmode == "pe":
            v = v + pe.double()[:l]                              # the table is indexed by the position INSIDE the sequence
        v = v.clone().requires_grad_(True)
        y = F.layer_norm(v, (D,), P64[0], P64[1], EPS) * m[rows]
        hh = F.conv1d(y.transpose(1, 2), P64[2], P64[3], padding=k // 2, groups=D).transpose(1, 2)      # zero padding at the sequence's own ends
        total = total + (hh * dh.double()[rows]).sum()
        leaves.append((rows, v))
        with torch.no_grad():
            h_ref[rows], s_ref[rows] = hh, v
            mu_ref[rows] = v.mean(-1)
            rs_ref[rows] = 1.0 / torch.sqrt(v.var(-1, unbiased=False) + EPS)
    total.backward()
    for rows, v in leaves:
        dv_ref[rows] = v.grad

    print("\n  ln_dwconv_rag %s: S %d rows %d" % (case, S, R))
    _hold("h", h[live_d], h_ref[live])
    _hold("mean", mean[live_d], mu_ref[live])
    _hold("rstd", rstd[live_d], rs_ref[live])
    if sum_out is not None:
        _hold("sum", sum_out[live_d], s_ref[live])
    for nm, t in (("h", h), ("mean", mean), ("rstd", rstd), ("sum", sum_out)):
        assert t is None or bool((t[gap_d] == SENT).all()), (nm, "a row between the sequences was written")

    # ---- backward: twice on one workspace (first filled with NaN bytes), then with dx_add ---------------------------------
    xin = (sum_out if sum_out is not None else xd).clone()
    mean_in, rstd_in = mean.clone(), rstd.clone()
    xin[gap_d], mean_in[gap_d], rstd_in[gap_d] = float("nan"), float("nan"), float("nan")
    wsb = lib.stage_ln_dwconv_bwd_ws_bytes(D, k)
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=dev)
    runs = []
    for add in (None, None, dxad):
        dx, dg, db_, dw, dc = sent(R, D), sent(D), sent(D), sent(D, 1, k), sent(D)
        _ok(lib.stage_ln_dwconv_rag_bwd(dhd.data_ptr(), xin.data_ptr(), mean_in.data_ptr(), rstd_in.data_ptr(), gd.data_ptr(), bd.data_ptr(), wd.data_ptr(),
                                        dx.data_ptr(), _p(add), dg.data_ptr(), db_.data_ptr(), dw.data_ptr(), dc.data_ptr(), seqt.data_ptr(), S, Lmax, D, k,
                                        p, seed, ws.data_ptr(), wsb, _st()), "stage_ln_dwconv_rag_bwd")
        torch.cuda.synchronize()
        runs.append((dx, dg, db_, dw, dc))
    for nm, t in zip(("dgamma", "dbeta", "dw", "db"), runs[0][1:]):
        assert bool(torch.isfinite(t).all()), (nm, "not finite: a row outside the sequences reached a parameter gradient")
    for a, c in zip(runs[0], runs[1]):
        assert torch.equal(a, c), "two launches on the same workspace differ"
    for a, c in zip(runs[0][1:], runs[2][1:]):
        assert torch.equal(a, c), "dx_add changed a parameter gradient"
    dx, dg, db_, dw, dc = runs[0]
    _hold("dx", dx[live_d], dv_ref[live])
    _hold("dx+add", runs[2][0][live_d], dv_ref[live] + dxa.double()[live])
    _hold("dgamma", dg, P64[0].grad)
    _hold("dbeta", db_, P64[1].grad)
    _hold("dw", dw, P64[2].grad)
    _hold("db", dc, P64[3].grad)
    assert bool((dx[gap_d] == SENT).all()) and bool((runs[2][0][gap_d] == SENT).all()), "a dx row between the sequences was written"


# =====================================================================================================================
# 4. / 5. statement rows: the product's own tables
# =====================================================================================================================
DUP_G, DUP_ROWS = 1, (1, 3)        # group 1 (Lv = 4): word 3 is a bit-identical copy of word 1 in every frame


def _statement_layout(dev, Lqa):
    """N, NA, Li = 3, 5, 6, halo 4.  Lqa = 40: Lc takes the values 5, 8, 9, 12, 16, 17, 33 and 40 (the eight-rows-in-flight loop of the
    masked max with a full, a short and an overlong last step); one statement with holes, one whose only valid word is its last, one
    without a valid word; an example with dead frames.  Lqa = 13: the same lengths cut at 13."""
    from tvqaplus_amd import ragged
    N, NA, Li = 3, 5, 6
    Lv = [1, 4, 5, 8, 12, 13, 29, 40, 36, 0, 12, 29, 5, 8, 13]
    qa = np.zeros((N * NA, Lqa), bool)
    for gi, l in enumerate(Lv):
        qa[gi, :min(l, Lqa)] = True
    qa[10, :] = False
    qa[10, min(12, Lqa) - 1] = True                              # its only valid word is the last one it keeps
    qa[11, [1, 2, 5, 9]] = False                                 # holes
    qa = qa.reshape(N, NA, Lqa)
    fl = np.ones((N, Li), bool)
    fl[1, [0, 3, 5]] = False                                     # dead frames
    fl[2, 2] = False
    tab = ragged.RaggedTables(qa, fl, 4)
    if Lqa == 40:
        assert set(int(v) for v in tab.Lc) == {0, 5, 8, 9, 12, 16, 17, 33, 40}
    lay = ragged.RaggedLayout(tab, dev)
    return tab, lay, torch.from_numpy(qa.reshape(N * NA, Lqa).astype(np.float32))


def _near_ties(w, dup=None):
    """w (len, D) fp64 masked values of one sequence -> bool (D): the two largest lie within TIE_GAP (``dup``: row that is a copy of an
    earlier one and does not count as a second value)"""
    if dup is not None:
        w = torch.cat([w[:dup], w[dup + 1:]])
    if w.shape[0] < 2:
        return torch.zeros(w.shape[1], dtype=torch.bool)
    top = torch.topk(w, 2, dim=0).values
    return (top[0] - top[1]) < TIE_GAP


@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
def test_ln_masked_max_rag_vs_fp64(hip_device, lib, with_res):
    dev, K, Lqa = hip_device, 128, 40
    tab, lay, qmask = _statement_layout(dev, Lqa)
    U, S, Rd = tab.U, tab.S, lay.out_rows
    g = torch.Generator().manual_seed(41)
    x, res = torch.randn(U, K, generator=g), torch.randn(U, K, generator=g)
    gamma, beta = 1.0 + 0.2 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
    dout = torch.randn(Rd, K, generator=g)
    seqs = [tuple(int(v) for v in r) for r in tab.seq]
    for s, l, gi, dense in seqs:
        if gi == DUP_G:
            x[s + DUP_ROWS[1]], res[s + DUP_ROWS[1]] = x[s + DUP_ROWS[0]], res[s + DUP_ROWS[0]]
    xd, resd, gd, bd, md = x.to(dev), (res.to(dev) if with_res else None), gamma.to(dev), beta.to(dev), qmask.to(dev)
    out = torch.full((Rd, K), SENT, device=dev)
    idx = torch.full((Rd, K), ISENT, dtype=torch.int32, device=dev)
    sum_out, mean, rstd = torch.full((U, K), SENT, device=dev), torch.full((U,), SENT, device=dev), torch.full((U,), SENT, device=dev)
    _ok(lib.stage_rag_fill_pooled(out.data_ptr(), idx.data_ptr(), Rd, K, _st()), "stage_rag_fill_pooled")
    _ok(lib.stage_ln_masked_max_rag_fwd(xd.data_ptr(), _p(resd), sum_out.data_ptr(), gd.data_ptr(), bd.data_ptr(), md.data_ptr(), out.data_ptr(),
                                        idx.data_ptr(), mean.data_ptr(), rstd.data_ptr(), lay.seq.data_ptr(), S, Lqa, K, EPS, _st()),
        "stage_ln_masked_max_rag_fwd")
    torch.cuda.synchronize()

    # ---- fp64, each sequence alone; the gradient from torch.argmax (first maximum) -------------------------------------
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    v_all = (x.double() + res.double()) if with_res else x.double()
    out_ref = torch.full((Rd, K), NEG, dtype=torch.float64)
    arg_ref = torch.zeros(Rd, K, dtype=torch.int64)
    tie = torch.zeros(Rd, K, dtype=torch.bool)
    live_out = torch.zeros(Rd, dtype=torch.bool)
    ys = []
    for s, l, gi, dense in seqs:
        v = v_all[s:s + l].clone().requires_grad_(True)
        y = F.layer_norm(v.unsqueeze(0), (K,), g64, b64, EPS)[0]
        mk = qmask[gi, :l].double()
        assert mk[:min(l, int(tab.Lv[gi]))].any() and not mk[int(tab.Lv[gi]):].any()        # the halo rows are masked
        wv = O.mask_logits(y, mk[:, None])
        arg = torch.argmax(wv.detach(), dim=0)
        out_ref[dense], arg_ref[dense], live_out[dense] = wv.detach()[arg, torch.arange(K)], arg, True
        tie[dense] = _near_ties(wv.detach(), DUP_ROWS[1] if gi == DUP_G else None)
        ys.append((s, l, dense, v, y, mk, arg))
    frac = float(tie[live_out].double().mean())
    print("\n  ln_masked_max_rag: U %d S %d near ties %.4f %% of %d pairs" % (U, S, 100 * frac, int(live_out.sum()) * K))
    assert frac <= 0.01
    dout[tie] = 0.0
    total = 0.0
    for s, l, dense, v, y, mk, arg in ys:
        dy = torch.zeros(l, K, dtype=torch.float64)
        dy[arg, torch.arange(K)] = dout[dense].double() * mk[arg]
        total = total + (y * dy).sum()
    total.backward()
    dv_ref = torch.zeros(U, K, dtype=torch.float64)
    for s, l, dense, v, y, mk, arg in ys:
        dv_ref[s:s + l] = v.grad

    _hold("out", out.cpu()[live_out], out_ref[live_out])
    assert bool((out.cpu()[~live_out] == NEG32).all()) and bool((idx.cpu()[~live_out] == 0).all())      # dead frames: the fill, untouched
    got_arg = idx.cpu().long()
    assert torch.equal(got_arg[live_out][~tie[live_out]], arg_ref[live_out][~tie[live_out]])
    dup_dense = [dense for s, l, gi, dense in seqs if gi == DUP_G]
    firsts = arg_ref[dup_dense] == DUP_ROWS[0]
    assert int(firsts.sum()) >= 10, "the duplicated row should be the maximum of some columns"
    assert bool((got_arg[dup_dense][firsts] == DUP_ROWS[0]).all()) and not bool((got_arg[dup_dense] == DUP_ROWS[1]).any())
    _hold("mean", mean, v_all.mean(-1))
    _hold("rstd", rstd, 1.0 / torch.sqrt(v_all.var(-1, unbiased=False) + EPS))
    if with_res:
        _hold("sum", sum_out, v_all)
    else:
        assert bool((sum_out == SENT).all())                     # nothing to export without a residual

    xin = sum_out if with_res else xd
    doutd = dout.to(dev)
    wsb = lib.stage_ln_bwd_ws_bytes(K)
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=dev)
    dx, dg, db_ = torch.full((U, K), float("nan"), device=dev), torch.full((K,), float("nan"), device=dev), torch.full((K,), float("nan"), device=dev)
    _ok(lib.stage_ln_masked_max_rag_bwd(doutd.data_ptr(), idx.data_ptr(), md.data_ptr(), xin.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gd.data_ptr(),
                                        dx.data_ptr(), dg.data_ptr(), db_.data_ptr(), lay.rowinfo.data_ptr(), U, K, ws.data_ptr(), wsb, _st()),
        "stage_ln_masked_max_rag_bwd")
    torch.cuda.synchronize()
    _hold("dx", dx, dv_ref)
    _hold("dgamma", dg, g64.grad)
    _hold("dbeta", db_, b64.grad)


# =====================================================================================================================
# 5. / 6. the encoder group on ragged rows
# =====================================================================================================================
def _block_params(D, k, n_conv, g):
    """the parameters of one encoder block in the order groups.encoder_block documents, and the oracle's names for them"""
    vals, names = [], []
    for i in range(n_conv):
        vals += [1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g), 0.5 * torch.randn(D, 1, k, generator=g),
                 0.1 * torch.randn(D, generator=g), 0.4 * torch.randn(D, D, 1, generator=g) / (D / 8) ** 0.5, 0.1 * torch.randn(D, generator=g)]
        names += [f"{KEY}.layer_norm.{i}.weight", f"{KEY}.layer_norm.{i}.bias", f"{KEY}.conv.{i}.depthwise_conv.weight",
                  f"{KEY}.conv.{i}.depthwise_conv.bias", f"{KEY}.conv.{i}.pointwise_conv.weight", f"{KEY}.conv.{i}.pointwise_conv.bias"]
    vals += [1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)]
    names += [KEY + ".final_layer_norm.weight", KEY + ".final_layer_norm.bias"]
    return names, vals


def _oracle_block(seqs, x, pe, names, vals, n_conv, p, seeds, qmask, Rd, dout):
    """oracle.encoder_block on each (1, len, D) sequence alone, in float64; pooled (qmask given): mask_logits and the first maximum over
    the words into the dense row, dead rows -1e10.  Returns out, dx, parameter gradients, near-tie pairs (pooled)."""
    U, D = x.shape
    dtype = torch.float64
    P = {n: v.detach().clone().to(dtype).requires_grad_(True) for n, v in zip(names, vals)}
    P[KEY + ".position_encoding.pe"] = pe.to(dtype)
    xl = x.detach().clone().to(dtype).requires_grad_(True)
    keep = [keep_mult(sd, p, U * D).view(U, D) for sd in seeds] if p > 0 else []
    # site order = the order the oracle draws in: ONE encoder_block call per sequence (outer loop), inside it one site per even conv
    # layer, which takes seeds[i // 2] as the group does.  Batching sequences into one call would change this order.
    sites = [keep[i // 2][s:s + l] for s, l, *_ in seqs for i in range(0, n_conv, 2)] if p > 0 else []
    pooled = qmask is not None
    out = torch.full((Rd, D), NEG, dtype=dtype) if pooled else torch.zeros(U, D, dtype=dtype)
    tie = torch.zeros(Rd, D, dtype=torch.bool) if pooled else None
    parts = []
    with O.drop_masks(sites):
        for s, l, gi, dense in seqs:
            y = O.encoder_block(xl[s:s + l].unsqueeze(0), torch.ones(1, l, dtype=dtype), P, KEY, n_conv, 0, p, True)[0]
            if pooled:
                wv = O.mask_logits(y, qmask[gi, :l].to(dtype)[:, None])
                arg = torch.argmax(wv.detach(), dim=0)
                y = wv[arg, torch.arange(D)]
                tie[dense] = _near_ties(wv.detach().double())
                out[dense] = y.detach()
                parts.append((y, dense))
            else:
                out[s:s + l] = y.detach()
                parts.append((y, slice(s, s + l)))
    if pooled:
        dout = dout.clone()
        dout[tie] = 0.0                                          # near ties carry no gradient (module docstring)
    total = sum((y * dout[where].to(dtype)).sum() for y, where in parts)
    total.backward()
    return out, xl.grad, [P[n].grad for n in names], tie, dout


def _encoder_group_vs_oracle(dev, lay, seqs, qmask, pe_rows, k, p, seed0):
    """groups.encoder_block_rag (D 128, two conv layers of width k) against the oracle in fp64: output, dx, every parameter gradient at TOL"""
    from tvqaplus_amd import groups
    from tvqaplus_amd.stage import _PositionTable
    D, n_conv = 128, 2
    U = lay.U
    pooled = qmask is not None
    Rd = lay.out_rows if pooled else U
    g = torch.Generator().manual_seed(seed0)
    names, vals = _block_params(D, k, n_conv, g)
    x = torch.randn(U, D, generator=g)
    pe = _PositionTable.table(pe_rows, D)
    dout = torch.randn(Rd, D, generator=g)
    seeds = [0x51DE5EED0001 + seed0]
    o64, dx64, gp64, tie, dout = _oracle_block(seqs, x, pe, names, vals, n_conv, p, seeds, qmask, Rd, dout)
    if pooled:
        live = torch.zeros(Rd, dtype=torch.bool)
        live[[dense for *_, dense in seqs]] = True
        frac = float(tie[live].double().mean())
        print("\n  near ties %.4f %% of %d pairs" % (100 * frac, int(live.sum()) * D))
        assert frac <= 0.01

    xd = x.to(dev).requires_grad_(True)
    params = [v.to(dev).requires_grad_(True) for v in vals]
    out = groups.encoder_block_rag(xd, pe.to(dev), None if qmask is None else qmask.to(dev), lay, k, p, seeds, params)
    assert tuple(out.shape) == (Rd, D)
    out.backward(dout.to(dev))
    torch.cuda.synchronize()
    if pooled:
        assert bool((out.detach()[~live.to(dev)] == NEG32).all())            # dead frames: the constant, exactly
    _hold("out", out.detach(), o64)
    _hold("dx", xd.grad, dx64)
    for n, q, r in zip(names, params, gp64):
        _hold(n[len(KEY) + 1:], q.grad, r)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("Lqa", [40, 13])
def test_encoder_group_rag_pooled_vs_fp64(hip_device, Lqa, p):
    """groups.encoder_block_rag with the masked max (the classifier encoder, D 128, two conv layers of width 5) against
    oracle.encoder_block + mask_logits + first maximum in fp64, each (1, Lc, D) sequence alone: pooled output, dx, every parameter gradient."""
    tab, lay, qmask = _statement_layout(hip_device, Lqa)
    seqs = [tuple(int(v) for v in r) for r in tab.seq]
    _encoder_group_vs_oracle(hip_device, lay, seqs, qmask, Lqa, 5, p, 100 + Lqa)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_encoder_group_rag_unpooled_on_a_context_layout_vs_fp64(hip_device, p):
    """groups.encoder_block_rag without pooling on a ragged context stream (the input encoder: two conv layers of width 7, halo 6; L = 60
    gives two chunks of 30, the kept lengths 7, 30, 31 and 60 end inside, on and behind the chunk edge): the (U, D) rows, dx, every
    parameter gradient against oracle.encoder_block in fp64 on each frame's rows alone."""
    from tvqaplus_amd import ragged
    N, Li, L, halo = 2, 8, 60, 6
    lens = np.array([[0, 1, 24, 25, 54, 60, 13, 0], [60, 2, 37, 25, 1, 48, 24, 9]])
    tab = ragged.CtxTables(lens, L, halo)
    assert {7, 30, 31, 60} <= set(int(v) for v in tab.seq[:, 1])
    lay = ragged.CtxLayout(tab, hip_device)
    seqs = [(int(r[0]), int(r[1]), 0, 0) for r in tab.seq]
    _encoder_group_vs_oracle(hip_device, lay, seqs, None, L, 7, p, 300)
