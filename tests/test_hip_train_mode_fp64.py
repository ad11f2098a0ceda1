"""The training-mode (DROP = true) instantiations of the dense per-op kernels, each held against a plain float64 restatement of the same
operation written HERE; no project kernel takes part in a reference.  The only shared piece is the host hash of the dropout stream
(``keep_mult`` of tests/test_hip_dropout_parity.py, pinned bit for bit to stage_dropout_keepmask): the keep multipliers are a pure
function of (seed, element index) (csrc/common.h: mix64 / drop4 / drop1), so a reference drops exactly the units a kernel drops.

    1  ops.mha_core                csrc/mha_mfma.hip mha_fwd/bwd_mfma_kernel<T, KS>, csrc/mha.hip mha_core_fwd/bwd_kernel
    2  ops.structured_attention    csrc/str_attn_fwd_reg.hip, str_attn_fwd.hip (d128, generic), str_attn_long.hip; l2norm_fwd/bwd<DROP> around them
    3  stage_layernorm_fwd/bwd     csrc/rowops.hip ln_fwd/bwd_fast_kernel<0, true, NQ 1..4>
    4  ops.cat3_layernorm          csrc/rowops.hip ln_fwd/bwd_fast_kernel<1, true>, ln_fwd/bwd_kernel<1, true>, cat3_ln_bwd_rep_kernel<true>
    5  ops.ln_dwconv               csrc/ln_dwconv.hip ln_dwconv_fwd/bwd_kernel<KT, true>
    6  stage_l2norm_fwd/bwd        csrc/rowops.hip l2norm_fwd/bwd_kernel<DROP>, accumulate 0 / 1
    7  ops.input_ln_linear         stage_layernorm_fwd + stage_gemm_nt_mask; stage_gemm_tn_mask + stage_dropout_keepmask + stage_gemm_nt_lnparam

Element index of the dropout stream (a test fails if one is off): row * K + col of the (rows, K) output for 3, 5, 6, 7; row * 3D + col
for 4; ((m * nh + h) * L + i) * L + j of the virtual (M, nh, L, L) probabilities for 1 (multiplier after the softmax, the softmax
backward on the pre-dropout probabilities); for 2 two streams: seed_c over the (N * NA * Lqa, D) normalised context rows, seed_q over
the (N * Li * Lr, D) normalised region rows.

Bounds.  Hard: 2e-4 under conftest.rel_err for every output and gradient (tests/test_hip_ops.py), 1e-3 for K1's dC / dQ (the eval-mode
K1 tests), tests/test_hip_bf16.py's ULP2 for the bf16 cases.  Second bound, "of scale" = max|got - ref| / max|ref| of a tensor:
16 x what a plain fp32 CPU evaluation of the same restatement is off fp64 on the cases of the family (the *_FP32 constants below,
each with its provenance; rule and the factor 16 as in tests/test_hip_cat3_fp64.py).  No family needed a bound of its own.  Measured
figures per entry point and what the file catches (mutated builds): docs/findings.md, finding 72.  The CPU tests at the end of the
file (not marked gpu) hold the references and the constants themselves.
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from oracle import stage_oracle as O
from test_hip_dropout_parity import keep_mult

TOL = 2e-4                      # tests/test_hip_ops.py: every kernel, outputs and gradients
TOL_K1G = 1e-3                  # tests/test_hip_ops.py: K1's dC / dQ (the scale-10 softmax backward cancels heavily)
ULP2 = 2 * 2.0 ** -8            # tests/test_hip_bf16.py: the bf16 storage bound of mha_core
EPS_LN = 1e-5
EPS_L2 = float(np.float32(1e-12))       # the float the kernels receive
NEG32 = float(np.float32(-1e10))
GUARD = 5                       # rows behind every C-ABI output that must keep the sentinel
SENT = -7777.25
BAND, BAND_CAP = 1e-4, 1e-3     # |pre64| < BAND * max|pre64| carries no claim about the ReLU bit; at most BAND_CAP of the elements
FACTOR = 16                     # fp16-pair products: 22 of fp32's 24 mantissa bits in two operands = 2^2 * 2^2 (test_hip_cat3_fp64.py)

# What a plain fp32 torch evaluation of each restatement below (same inputs, same keep multipliers, CPU, ONE thread: torch's reductions
# over many rows split by thread count, one thread is the plain sequential sum and repeats everywhere) is off the float64 one, of
# scale: worst tensor of the worst case of the family's case list, rounded up.  The CPU tests at the end assert the smallest case
# from above and the worst case from both sides (a constant may not be more than a tenth above its figure).
MHA_FP32 = 8.0e-7         # 7.99e-7 at (2, 64, 64, 1) p 0.3; the other cases 2.0e-7 .. 5.6e-7, L = 1: 4.1e-8
K1_FP32 = 8.2e-7          # 8.16e-7 at Lr 100, D 32; 6.9e-7 at Lr 50, 6.4e-7 at Lr 77; the others 3.7e-7 .. 5.3e-7
LN_FP32 = 1.7e-7          # 1.69e-7 at K 1024 p 0.5; 1.1e-7 .. 1.7e-7 everywhere, 33 001 rows included (torch sums those pairwise)
CAT3_FP32 = 4.9e-7        # 4.81e-7 at (2, 3, 40, 128); 1.4e-7 .. 2.8e-7 for the three small cases
LNDW_FP32 = 4.2e-7        # 4.18e-7 at (5, 40, 128, 5); the cases up to 490 rows 1.4e-7 .. 4.2e-7; h, sum, dx, dres, db of (300, 40, 128, 5) <= 3.2e-7
LNDW_ROWS_FP32 = 2.7e-6   # dgamma, dbeta, dw of (300, 40, 128, 5) alone: 2.70e-6, 1.21e-6, 6.1e-7 -- torch's sequential fp32 sums over 12 000 rows
LNDW_ROW_SUMS = ("dgamma", "dbeta", "dw")
L2_FP32 = 1.6e-7          # 1.56e-7 at K 300 p 0.3; 9.1e-8 .. 1.6e-7
MLP_FP32 = 2.1e-6         # 2.03e-6 at (9000, 128, 72); 1.6e-6 .. 1.9e-6 for the others: column sums over 4100 .. 9000 rows


# ---- helpers ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops(request):
    """the product's op wrappers; without a GPU the tests of this file that need one skip (a run that asks for `-m gpu` fails loudly)"""
    if not torch.cuda.is_available() and "gpu" not in (request.config.getoption("-m") or ""):
        pytest.skip("needs a GPU")
    request.getfixturevalue("hip_device")
    from tvqaplus_amd import _lib
    from tvqaplus_amd import ops as _ops
    assert _lib.load().stage_hip_abi_version() == _lib.ABI_VERSION
    return _ops


def _st():
    return torch.cuda.current_stream().cuda_stream


def _id(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def _keep(seed, p, shape):
    """multipliers (0 or 1 / (1 - p)) of stream ``seed`` for a tensor of ``shape``: element index = the flat index"""
    n = int(np.prod(shape))
    return keep_mult(seed, p, n).view(shape) if p > 0 else torch.ones(shape)


def _scale_err(got, ref):
    ref = ref.detach().double().cpu()
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    s = float(ref.abs().max()) if ref.numel() else 0.0
    return float((got - ref).abs().max()) / (s if s > 0 else 1.0) if ref.numel() else 0.0     # an all-zero reference: absolute


def _hold(fam, name, got, ref, tol=TOL, stol=None):
    """finite, within tol of the fp64 reference under rel_err and within stol of scale; prints both figures (run with -s to collect)"""
    assert bool(torch.isfinite(got).all()), (fam, name, "not finite")
    e, s = rel_err(got.float(), ref), _scale_err(got, ref)
    print("    %-22s %-8s rel_err %.3e  of_scale %.3e" % (fam, name, e, s))
    assert e < tol, (fam, name, "rel_err", e, tol)
    assert stol is None or s <= stol, (fam, name, "of scale", s, stol)
    return s


def _kept_ok(keep, p):
    """kept fraction of a rebuilt mask within 5 sigma of 1 - p"""
    n = keep.numel()
    frac = float((keep != 0).double().mean())
    return abs(frac - (1.0 - p)) <= 5.0 * math.sqrt(p * (1.0 - p) / n) + 1e-5, frac     # (+1e-5: the threshold is round(p * 65536) / 65536)


def _worst(r32, r64, names):
    return max(_scale_err(r32[k], r64[k]) for k in names if r64.get(k) is not None)


class _Out:
    """a device tensor of ``rows`` rows with GUARD sentinel rows behind it"""

    def __init__(self, rows, cols, fill=float("nan")):
        self.rows = rows
        self.buf = torch.full((rows + GUARD, cols) if cols else (rows + GUARD,), fill, dtype=torch.float32, device="cuda")
        self.buf[rows:] = SENT
        self.t = self.buf[:rows]

    def ptr(self):
        return self.buf.data_ptr()

    def guard_ok(self):
        return bool((self.buf[self.rows:] == SENT).all())


def _p(t):
    return None if t is None else t.data_ptr()


def _leaf(t, dt, grad=True):
    """a fresh leaf of dtype ``dt`` (the cached problem tensors are never touched)"""
    return t.detach().to(dt).clone().requires_grad_(grad)


def _dev(t, grad=False):
    return t.detach().clone().cuda().requires_grad_(grad)


# =====================================================================================================================
# 1. multi-head attention core with dropout of the probabilities
# =====================================================================================================================
# (M, L, D, nh, p): every head width dk = D / nh in {8, 16, 32, 64} (KS 2, 4, 8, 16 of MHA_DISPATCH) and every tile count T = ceil(L / 16)
# in 1..4, L on and beside the tile edges; a workgroup holds four (m, h) items, M * nh = 12, 10, 8, 6, 2 leave the last one partly filled
MHA_MFMA = [(3, 16, 32, 4, 0.1),     # dk 8,  T 1, L on the tile edge
            (3, 17, 64, 4, 0.3),     # dk 16, T 2, one row into the second tile
            (5, 15, 16, 2, 0.1),     # dk 8,  T 1, one row short; 10 items
            (2, 33, 128, 4, 0.1),    # dk 32, T 3
            (3, 48, 128, 4, 0.3),    # dk 32, T 3, on the edge
            (2, 49, 32, 1, 0.1),     # dk 32, T 4; 2 items
            (2, 64, 64, 1, 0.3),     # dk 64, T 4, the largest L
            (3, 32, 128, 2, 0.1),    # dk 64, T 2, on the edge; 6 items
            (5, 1, 16, 2, 0.3)]      # L 1: dq and dk are exactly zero
# the matrix-core kernels decline these: mha_core_fwd/bwd_kernel (csrc/mha.hip) run without the developer switch
MHA_SCALAR = [(3, 20, 24, 2, 0.1),   # dk 12
              (3, 17, 8, 2, 0.3)]    # dk 4
MHA_BF16 = [(3, 17, 64, 4, 0.3), (2, 33, 128, 4, 0.1)]
MHA_SEED = 0x5EEDC0DE1234


@functools.lru_cache(maxsize=None)
def _mha_problem(case, bf16=False):
    M, L, D, nh, p = case
    g = torch.Generator().manual_seed(M * 1000 + L * 10 + nh)
    q, k, v, go = (torch.randn(M, L, D, generator=g) for _ in range(4))
    if bf16:
        q, k, v, go = (t.to(torch.bfloat16).float() for t in (q, k, v, go))
    lens = torch.randint(1, max(L, 2), (M,), generator=g)            # ragged
    lens[0] = L                                                      # a full sequence
    if M >= 3:
        lens[M - 1] = 0                                              # a sequence without a valid row: every query row attends uniformly
    else:
        lens[1] = L // 3
    mask = (torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)).float()
    return dict(q=q, k=k, v=v, go=go, mask=mask, keep=_keep(MHA_SEED, p, (M, nh, L, L)))


def _mha_restate(case, pr, dt):
    """model/self_attention.py:56-71 with the query-row quirk of oracle.multi_head_attention: padded QUERY rows get -1e9 (uniform
    attention), padded keys are not masked; the multiplier after the softmax"""
    M, L, D, nh, p = case
    dk = D // nh
    q, k, v = (_leaf(pr[n], dt) for n in "qkv")
    sp = lambda t: t.view(M, L, nh, dk).transpose(1, 2)
    s = torch.matmul(sp(q), sp(k).transpose(-2, -1)) / math.sqrt(dk)
    s = s.masked_fill(pr["mask"].view(M, 1, L, 1) == 0, -1e9)
    pd = torch.softmax(s, -1) * pr["keep"].to(dt)
    out = torch.matmul(pd, sp(v)).transpose(1, 2).reshape(M, L, D)
    out.backward(pr["go"].to(dt))
    return dict(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


@functools.lru_cache(maxsize=None)
def _mha_ref(case, bf16=False):
    return _mha_restate(case, _mha_problem(case, bf16), torch.float64)


def _mha_run(ops, case, pr, dt):
    M, L, D, nh, p = case
    qd, kd, vd = (pr[n].to(dt).cuda().requires_grad_() for n in "qkv")
    o = ops.mha_core(qd, kd, vd, pr["mask"].cuda(), nh, p=p, seed=MHA_SEED)
    o.backward(pr["go"].to(dt).cuda())
    torch.cuda.synchronize()
    return dict(out=o.detach(), dq=qd.grad, dk=kd.grad, dv=vd.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("case", MHA_MFMA + MHA_SCALAR, ids=_id)
def test_mha_core_with_dropout_against_fp64(ops, case):
    M, L, D, nh, p = case
    assert ops._lib.load().stage_mha_core_recomputes(L, D, nh) == (1 if case in MHA_MFMA else 0)
    pr, ref = _mha_problem(case), _mha_ref(case)
    if L == 1:
        assert not bool(ref["dq"].any()) and not bool(ref["dk"].any())
    got = _mha_run(ops, case, pr, torch.float32)
    for n in ("out", "dq", "dk", "dv"):                  # (an all-zero reference compares absolutely under both measures)
        _hold("mha %s" % _id(case), n, got[n], ref[n], TOL, FACTOR * MHA_FP32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", MHA_BF16, ids=_id)
def test_mha_core_with_dropout_bf16_storage_against_fp64(ops, case):
    """bf16 q / k / v / dout: the reference gets the bf16-rounded inputs; the bound of tests/test_hip_bf16.py's test_mha_core_bf16"""
    pr, ref = _mha_problem(case, True), _mha_ref(case, True)
    got = _mha_run(ops, case, pr, torch.bfloat16)
    for n in ("out", "dq", "dk", "dv"):
        assert got[n].dtype == torch.bfloat16
        _hold("mha bf16 %s" % _id(case), n, got[n], ref[n], ULP2)


# =====================================================================================================================
# 2. K1 (StructuredAttention) in training mode: dropout of the normalised context rows and of the normalised region rows
# =====================================================================================================================
# (N, Li, Lr, Lqa, D, long)
K1_CASES = [(2, 3, 20, 40, 128, False),     # register kernel (Lr <= 32), fused backward
            (1, 3, 32, 13, 128, False),     # register kernel at its largest Lr
            (1, 3, 33, 23, 128, False),     # LDS-staged kernel (32 < Lr <= 64); odd Lr: three-kernel backward
            (2, 3, 50, 40, 128, False),     # LDS-staged kernel, fused backward
            (1, 3, 64, 13, 128, False),     # LDS-staged kernel at its largest Lr
            (1, 3, 25, 23, 128, False),     # register kernel, odd Lr: the backward takes the three-kernel path
            (1, 3, 25, 13, 32, False),      # generic kernels (D != 128)
            (1, 3, 77, 23, 128, True),      # str_attn_long_*: five 16-region blocks, the last partly filled
            (1, 3, 100, 13, 32, True)]      # str_attn_long_* at D 32
K1_P, K1_SCALE, K1_SEED_C, K1_SEED_Q = 0.3, 10.0, 77, 4242
K1_NAMES = ("A", "S", "Sn", "dC", "dQ")


@functools.lru_cache(maxsize=None)
def _k1_problem(case):
    from tvqaplus_amd.synth import make_batch
    N, Li, Lr, Lqa, D, _ = case
    g = torch.Generator().manual_seed(1000 + Lr + D)
    b = make_batch(N=N, Li=Li, Lr=Lr, Lw=2, Lqa=Lqa, wd_size=4, vfeat_size=4, seed=Lr + Lqa, empty_frames=True)
    return dict(C=torch.randn(N, 5, 1, Lqa, D, generator=g), Q=torch.randn(N, 1, Li, Lr, D, generator=g) * 2,
                cm=b.qas_mask.view(N, 5, 1, Lqa), qm=b.vid_mask.view(N, 1, Li, Lr),
                gA=torch.randn(N, 5, Li, Lqa, D, generator=g), gS=torch.randn(N, 5, Li, Lqa, Lr, generator=g) * 0.1,
                keeps=[_keep(K1_SEED_C, K1_P, (N * 5 * Lqa, D)), _keep(K1_SEED_Q, K1_P, (N * Li * Lr, D))])


def _k1_restate(pr, dt):
    """oracle.structured_attention in ``dt`` with the two rebuilt masks, in its visiting order: context rows, then region rows"""
    C, Q = _leaf(pr["C"], dt), _leaf(pr["Q"], dt)
    with O.drop_masks(pr["keeps"]):
        A, S, Sm, Sn = O.structured_attention(C, Q, pr["cm"].to(dt), pr["qm"].to(dt), K1_SCALE, K1_P, True)
    ((A * pr["gA"].to(dt)).sum() + (S * pr["gS"].to(dt)).sum()).backward()
    live = Sm != 0
    return dict(A=A.detach(), S=S.detach() * live, Sn=Sn.detach(), dC=C.grad, dQ=Q.grad, live=live)      # S: the unmasked entries


@functools.lru_cache(maxsize=None)
def _k1_ref(case):
    return _k1_restate(_k1_problem(case), torch.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("case", K1_CASES, ids=_id)
def test_k1_training_mode_against_fp64(ops, case):
    N, Li, Lr, Lqa, D, long_rows = case
    pr, ref = _k1_problem(case), _k1_ref(case)
    Cd, Qd = _dev(pr["C"].view(N, 5, Lqa, D), True), _dev(pr["Q"].view(N, Li, Lr, D), True)
    fn = ops.structured_attention_long if long_rows else ops.structured_attention
    A, S, Sn = fn(Cd, Qd, pr["cm"].view(N, 5, Lqa).cuda(), pr["qm"].view(N, Li, Lr).cuda(), K1_SCALE, p=K1_P, seed_c=K1_SEED_C, seed_q=K1_SEED_Q)
    ((A * pr["gA"].cuda()).sum() + (S * pr["gS"].cuda()).sum()).backward()
    torch.cuda.synchronize()
    live = ref["live"]
    assert 0.05 < float(live.double().mean()) < 0.95
    assert bool((S.detach().cpu()[~live] == NEG32).all())            # masked scores: the fp32 constant, exactly
    assert float((A == 0).float().mean()) < 0.9                      # not a degenerate all-masked case
    got = dict(A=A.detach(), S=S.detach().cpu() * live, Sn=Sn.detach(), dC=Cd.grad.view_as(pr["C"]), dQ=Qd.grad.view_as(pr["Q"]))
    for n in K1_NAMES:
        _hold("k1 %s" % _id(case[:5]), n, got[n], ref[n], TOL_K1G if n in ("dC", "dQ") else TOL, FACTOR * K1_FP32)


# =====================================================================================================================
# 3. LayerNorm (+ residual / position table) with dropout, through the C ABI
# =====================================================================================================================
# (rows, K, variant, p).  K / 4 quads over LPR = min(64, pow2ceil(K / 4)) lanes, NQ = ceil(K / 4 / LPR) quads per lane (ln_fwd_launch):
#   K 16: LPR 4 NQ 1 | 48: LPR 16 NQ 1, four lanes idle | 128: LPR 32 | 256: LPR 64 NQ 1 | 300: NQ 2, the second quad on 11 lanes only |
#   768: NQ 3 | 1024: NQ 4.  37 rows never fill the last block (4 * 64 / LPR rows per block).  Each K meets both rates; the residual
#   variant rotates: none, a full residual (res_period 0), a position table (res_period L = 5).
LN_VARIANTS = ("none", "full", "pe")
LN_KS = (16, 48, 128, 256, 300, 768, 1024)
LN_CASES = [(37, K, LN_VARIANTS[(i + j) % 3], p) for i, K in enumerate(LN_KS) for j, p in enumerate((0.1, 0.5))]
LN_CASES += [(33001, 128, "full", 0.1)]      # 4126 blocks of 8 rows: the backward's 512-block grid walks nine times, colreduce adds 512 partials
LN_PE_L = 5
LN_SEED = 0x1234ABCD77
LN_NAMES = ("y", "sum", "mean", "rstd", "dx", "dgamma", "dbeta")


@functools.lru_cache(maxsize=4)
def _ln_problem(case):
    rows, K, var, p = case
    g = torch.Generator().manual_seed(rows * 1000 + K)
    pr = dict(x=torch.randn(rows, K, generator=g) * 2 + 0.5, gamma=1 + 0.3 * torch.randn(K, generator=g), beta=0.3 * torch.randn(K, generator=g),
              dy=torch.randn(rows, K, generator=g), dsum=torch.randn(rows, K, generator=g), keep=_keep(LN_SEED, p, (rows, K)), res=None)
    if var != "none":
        pr["res"] = torch.randn((rows, K) if var == "full" else (LN_PE_L + 3, K), generator=g)
    return pr


def _ln_restate(case, pr, dt):
    """y = drop(LN(x + res)), the exported sum x + res; a gradient arrives on y and on the exported sum.  dres of a full residual is dx."""
    rows, K, var, p = case
    x, gamma, beta = (_leaf(pr[n], dt) for n in ("x", "gamma", "beta"))
    v = x
    if var == "full":
        v = x + pr["res"].to(dt)
    elif var == "pe":
        v = x + pr["res"].to(dt)[torch.arange(rows) % LN_PE_L]
    mu = v.mean(-1, keepdim=True)
    rstd = (((v - mu) ** 2).mean(-1, keepdim=True) + EPS_LN) ** -0.5
    y = ((v - mu) * rstd * gamma + beta) * pr["keep"].to(dt)
    loss = (y * pr["dy"].to(dt)).sum()
    if var != "none":
        loss = loss + (v * pr["dsum"].to(dt)).sum()
    loss.backward()
    return dict(y=y.detach(), sum=v.detach() if var != "none" else None, mean=mu.detach().squeeze(1), rstd=rstd.detach().squeeze(1),
                dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, v=v.detach())


@pytest.mark.gpu
@pytest.mark.parametrize("case", LN_CASES, ids=_id)
def test_layernorm_with_dropout_against_fp64(ops, case):
    """stage_layernorm_fwd, then stage_layernorm_bwd on the fp64 reference's x + res, mean and rstd rounded to fp32 (no forward kernel
    stands behind the backward): y, exported sum, mean, rstd, dx (= dres of a full residual), dgamma, dbeta; guard rows; dropped elements"""
    from tvqaplus_amd import _lib
    lib = _lib.load()
    rows, K, var, p = case
    pr, ref = _ln_problem(case), _ln_restate(case, _ln_problem(case), torch.float64)
    stol = FACTOR * LN_FP32
    fam = "layernorm %s" % _id(case)
    xd, gd, bd = (pr[n].cuda() for n in ("x", "gamma", "beta"))
    resd = None if pr["res"] is None else pr["res"].cuda()
    y, mean, rstd = _Out(rows, K), _Out(rows, 0), _Out(rows, 0)
    s = _Out(rows, K) if var != "none" else None
    _lib.check(lib.stage_layernorm_fwd(xd.data_ptr(), _p(resd), LN_PE_L if var == "pe" else 0, None if s is None else s.ptr(), gd.data_ptr(),
                                       bd.data_ptr(), y.ptr(), mean.ptr(), rstd.ptr(), rows, K, EPS_LN, p, LN_SEED, _st()), "stage_layernorm_fwd")
    torch.cuda.synchronize()
    outs = dict(y=y, mean=mean, rstd=rstd)
    if s is not None:
        outs["sum"] = s
    for n, o in outs.items():
        assert o.guard_ok(), n
        _hold(fam, n, o.t, ref[n], TOL, stol)
    assert torch.equal((y.t == 0).cpu(), pr["keep"] == 0)            # the dropped elements are the ones the stream names: row * K + col

    xin, m32, r32 = ref["v"].float().cuda(), ref["mean"].float().cuda(), ref["rstd"].float().cuda()
    dyd = pr["dy"].cuda()
    dadd = pr["dsum"].cuda() if var != "none" else None
    wsb = lib.stage_ln_bwd_ws_bytes(K)
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device="cuda")
    dx, dg, db = _Out(rows, K), _Out(K, 0), _Out(K, 0)
    _lib.check(lib.stage_layernorm_bwd(dyd.data_ptr(), xin.data_ptr(), m32.data_ptr(), r32.data_ptr(), gd.data_ptr(), dx.ptr(), _p(dadd), dg.ptr(),
                                       db.ptr(), rows, K, p, LN_SEED, ws.data_ptr(), wsb, _st()), "stage_layernorm_bwd")
    torch.cuda.synchronize()
    for n, o in (("dx", dx), ("dgamma", dg), ("dbeta", db)):
        assert o.guard_ok(), n
        _hold(fam, n, o.t, ref[n], TOL, stol)


# =====================================================================================================================
# 4. LayerNorm over [a, b, a*b] with dropout, the unfused op (below 4096 rows the product falls back to it)
# =====================================================================================================================
# (G, rep, inner, D)
CAT3_CASES = [(3, 1, 5, 16),       # rep 1: ln_fwd/bwd_fast_kernel<1, true> (D / 4 == LPR == 4), da unreduced
              (3, 2, 5, 24),       # D / 4 = 6 != LPR = 8: the slow ln_fwd/bwd_kernel<1, true>, then stage_reduce_rep
              (4, 6, 7, 32),       # rep > 1: cat3_ln_bwd_rep_kernel<true>, LPR 8
              (2, 3, 40, 128)]     # rep > 1: cat3_ln_bwd_rep_kernel<true>, LPR 32 (the model's shape)
CAT3_P, CAT3_SEED = 0.1, 0x0C0FFEE123
CAT3_NAMES = ("y", "da", "db", "dgamma", "dbeta")


@functools.lru_cache(maxsize=None)
def _cat3_problem(case):
    G, rep, inner, D = case
    g = torch.Generator().manual_seed(G * 100 + rep + D)
    rows = G * rep * inner
    return dict(a=torch.randn(G * inner, D, generator=g), b=torch.randn(rows, D, generator=g), gamma=1 + 0.3 * torch.randn(3 * D, generator=g),
                beta=0.3 * torch.randn(3 * D, generator=g), dy=torch.randn(rows, 3 * D, generator=g), keep=_keep(CAT3_SEED, CAT3_P, (rows, 3 * D)))


def _cat3_restate(case, pr, dt):
    G, rep, inner, D = case
    a, b, gamma, beta = (_leaf(pr[n], dt) for n in ("a", "b", "gamma", "beta"))
    ae = a.view(G, 1, inner, D).expand(G, rep, inner, D).reshape(-1, D)
    y = F.layer_norm(torch.cat([ae, b, ae * b], -1), (3 * D,), gamma, beta, EPS_LN) * pr["keep"].to(dt)
    y.backward(pr["dy"].to(dt))
    return dict(y=y.detach(), da=a.grad, db=b.grad, dgamma=gamma.grad, dbeta=beta.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CAT3_CASES, ids=_id)
def test_cat3_layernorm_with_dropout_against_fp64(ops, case):
    G, rep, inner, D = case
    pr, ref = _cat3_problem(case), _cat3_restate(case, _cat3_problem(case), torch.float64)
    ad, bd, gd, btd = (_dev(pr[n], True) for n in ("a", "b", "gamma", "beta"))
    y = ops.cat3_layernorm(ad, bd, gd, btd, rep=rep, inner=inner, p=CAT3_P, seed=CAT3_SEED)
    y.backward(pr["dy"].cuda())
    torch.cuda.synchronize()
    assert torch.equal((y == 0).cpu(), pr["keep"] == 0)              # element index row * 3D + col
    got = dict(y=y.detach(), da=ad.grad, db=bd.grad, dgamma=gd.grad, dbeta=btd.grad)
    for n in CAT3_NAMES:
        _hold("cat3_layernorm %s" % _id(case), n, got[n], ref[n], TOL, FACTOR * CAT3_FP32)


# =====================================================================================================================
# 5. LayerNorm (+ residual / position table, + dropout) -> depthwise conv, dense
# =====================================================================================================================
# (M, L, D, k, period, p); period: -1 no residual, 0 a full residual, L a position table.  The shapes of
# test_ln_dwconv_fused_matches_unfused (tests/test_hip_ops.py), each with p > 0; then the outer widths and sequences shorter than the halo
LNDW_CASES = [(3, 5, 16, 7, 0, 0.1),          # KT 7, window wider than the sequence
              (6, 20, 128, 7, 20, 0.1),       # the input encoder's shape, position table
              (5, 40, 128, 5, 0, 0.25),       # the classifier encoder's shape
              (2, 33, 32, 3, -1, 0.1),        # KT 3, no residual and no exported sum
              (7, 70, 128, 5, 0, 0.25),
              (4, 9, 64, 9, 9, 0.1),          # KT 9, position table
              (300, 40, 128, 5, 0, 0.1),      # 12 000 rows: the backward's capped grid walks, column partials are reduced
              (5, 6, 32, 1, -1, 0.1),         # KT 1: no halo at all
              (4, 1, 32, 9, 0, 0.25),         # L 1: every tap but the centre falls outside
              (3, 2, 16, 5, 2, 0.1)]          # L 2 < k / 2 + 1, position table of two rows
LNDW_SEED = 1234
LNDW_NAMES = ("h", "sum", "dx", "dres", "dgamma", "dbeta", "dw", "db")


@functools.lru_cache(maxsize=2)
def _lndw_problem(case):
    M, L, D, k, period, p = case
    g = torch.Generator().manual_seed(M * L + k + D)
    pr = dict(x=torch.randn(M, L, D, generator=g), gamma=1 + 0.3 * torch.randn(D, generator=g), beta=0.3 * torch.randn(D, generator=g),
              w=0.5 * torch.randn(D, 1, k, generator=g), b=0.2 * torch.randn(D, generator=g), gh=torch.randn(M, L, D, generator=g),
              gs=torch.randn(M, L, D, generator=g), keep=_keep(LNDW_SEED, p, (M, L, D)), res=None)       # element index row * D + col, row = m * L + l
    if period >= 0:
        pr["res"] = torch.randn((M, L, D) if period == 0 else (L, D), generator=g)
    return pr


def _lndw_restate(case, pr, dt):
    """F.layer_norm -> keep -> F.conv1d(padding = k // 2, groups = D); a gradient arrives on h and on the exported sum"""
    M, L, D, k, period, p = case
    x, gamma, beta, w, b = (_leaf(pr[n], dt) for n in ("x", "gamma", "beta", "w", "b"))
    res = None if period < 0 else _leaf(pr["res"], dt, period == 0)
    v = x if res is None else x + res
    y = F.layer_norm(v, (D,), gamma, beta, EPS_LN) * pr["keep"].to(dt)
    h = F.conv1d(y.transpose(1, 2), w, b, padding=k // 2, groups=D).transpose(1, 2)
    loss = (h * pr["gh"].to(dt)).sum()
    if res is not None:
        loss = loss + (v * pr["gs"].to(dt)).sum()
    loss.backward()
    return dict(h=h.detach(), sum=None if res is None else v.detach(), dx=x.grad, dres=res.grad if period == 0 else None,
                dgamma=gamma.grad, dbeta=beta.grad, dw=w.grad, db=b.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LNDW_CASES, ids=_id)
def test_ln_dwconv_with_dropout_against_fp64(ops, case):
    M, L, D, k, period, p = case
    assert ops.ln_dwconv_supported(D, k)
    pr, ref = _lndw_problem(case), _lndw_restate(case, _lndw_problem(case), torch.float64)
    xd, gd, bd, wd, cd = (_dev(pr[n], True) for n in ("x", "gamma", "beta", "w", "b"))
    rd = None if period < 0 else _dev(pr["res"], period == 0)
    h, s = ops.ln_dwconv(xd, gd, bd, wd, cd, p=p, seed=LNDW_SEED, res=rd, res_period=max(period, 0))
    loss = (h * pr["gh"].cuda()).sum()
    if s is not None:
        loss = loss + (s * pr["gs"].cuda()).sum()
    loss.backward()
    torch.cuda.synchronize()
    got = dict(h=h.detach(), sum=None if s is None else s.detach(), dx=xd.grad, dres=rd.grad if period == 0 else None, dgamma=gd.grad,
               dbeta=bd.grad, dw=wd.grad, db=cd.grad)
    for n in LNDW_NAMES:
        if ref[n] is None:
            assert got[n] is None, n
            continue
        _hold("ln_dwconv %s" % _id(case), n, got[n], ref[n], TOL, FACTOR * (LNDW_ROWS_FP32 if M * L > 1000 and n in LNDW_ROW_SUMS else LNDW_FP32))


# =====================================================================================================================
# 6. l2norm forward and backward (+ dropout), through the C ABI
# =====================================================================================================================
# (rows, K, p): K 16 LPR 4 | 128 LPR 32 | 300 LPR 64, two quads per lane, the second on 11 lanes; 37 rows never fill the last block
L2_CASES = [(37, K, p) for K in (16, 128, 300) for p in (0.0, 0.3)]
L2_ZERO_ROW = 5                 # an all-zero row: n = max(|x|, eps) = eps, y = 0, dx = g / eps
L2_SEED = 0x77AA55
L2_NAMES = ("y", "norm", "dx")


@functools.lru_cache(maxsize=None)
def _l2_problem(case):
    rows, K, p = case
    g = torch.Generator().manual_seed(rows + K)
    x = torch.randn(rows, K, generator=g) * 3
    x[L2_ZERO_ROW] = 0.0
    return dict(x=x, dy=torch.randn(rows, K, generator=g), pre=torch.randn(rows, K, generator=g), keep=_keep(L2_SEED, p, (rows, K)))


def _l2_restate(case, pr, dt):
    """F.normalize(p = 2, eps) -> keep.  The clamped row's norm is a constant: its gradient is g / eps (what autograd gives for clamp_min)."""
    x = _leaf(pr["x"], dt)
    n = x.norm(dim=-1, keepdim=True).clamp_min(EPS_L2)
    y = (x / n) * pr["keep"].to(dt)
    y.backward(pr["dy"].to(dt))
    return dict(y=y.detach(), norm=n.detach().squeeze(1), dx=x.grad)


def _l2_live(t):
    """rows other than the clamped one (whose dx is of scale 1 / eps = 1e12 and is compared on its own)"""
    sel = torch.ones(t.shape[0], dtype=torch.bool)
    sel[L2_ZERO_ROW] = False
    return t.detach().cpu()[sel]


@pytest.mark.gpu
@pytest.mark.parametrize("case", L2_CASES, ids=_id)
def test_l2norm_forward_and_backward_against_fp64(ops, case):
    from tvqaplus_amd import _lib
    lib = _lib.load()
    rows, K, p = case
    pr, ref = _l2_problem(case), _l2_restate(case, _l2_problem(case), torch.float64)
    stol = FACTOR * L2_FP32
    fam = "l2norm %s" % _id(case)
    xd, dyd = pr["x"].cuda(), pr["dy"].cuda()
    y, nrm = _Out(rows, K), _Out(rows, 0)
    _lib.check(lib.stage_l2norm_fwd(xd.data_ptr(), y.ptr(), nrm.ptr(), rows, K, EPS_L2, p, L2_SEED, _st()), "stage_l2norm_fwd")
    torch.cuda.synchronize()
    assert y.guard_ok() and nrm.guard_ok()
    _hold(fam, "y", y.t, ref["y"], TOL, stol)
    _hold(fam, "norm", nrm.t, ref["norm"], TOL, stol)
    assert bool((y.t[L2_ZERO_ROW] == 0).all()) and float(nrm.t[L2_ZERO_ROW]) == EPS_L2
    if p > 0:
        live = torch.ones(rows, dtype=torch.bool)
        live[L2_ZERO_ROW] = False
        assert torch.equal((y.t == 0).cpu()[live], (pr["keep"] == 0)[live])          # element index row * K + col
    for acc in (0, 1):
        dx = _Out(rows, K)
        if acc:
            dx.t.copy_(pr["pre"].cuda())
        _lib.check(lib.stage_l2norm_bwd(dyd.data_ptr(), xd.data_ptr(), dx.ptr(), rows, K, EPS_L2, p, L2_SEED, acc, _st()), "stage_l2norm_bwd")
        torch.cuda.synchronize()
        assert dx.guard_ok()
        exp = ref["dx"] + (pr["pre"].double() if acc else 0.0)
        _hold(fam, "dx acc %d" % acc, _l2_live(dx.t), _l2_live(exp), TOL, stol)
        z = dx.t[L2_ZERO_ROW].double().cpu()                       # the clamped row, relative to its own 1e12 scale
        ez = exp[L2_ZERO_ROW]
        assert bool(torch.isfinite(z).all()) and float((z - ez).abs().max()) <= stol * float(ez.abs().max())


# =====================================================================================================================
# 7. the first layer of the input MLPs: LayerNorm -> dropout -> Linear -> ReLU on features that need no gradient
# =====================================================================================================================
# (M, K, N, p): the shapes of test_input_ln_linear_fused_backward (tests/test_hip_ops.py), each with p > 0
MLP_CASES = [(4200, 768, 300, 0.1),      # the subtitle stream's input width: NQ 3 LayerNorm, lnparam epilogue over 768 columns
             (5000, 300, 300, 0.1),      # the video stream's input width: NQ 2 with a partly filled quad
             (9000, 128, 72, 0.25),      # N no multiple of 32: the last mask word partly filled
             (4100, 260, 128, 0.1)]      # K no multiple of 64 (the smallest case: the CPU test's)
MLP_SEED = 1234567
MLP_NAMES = ("y", "dgamma", "dbeta", "dW", "db")


@functools.lru_cache(maxsize=1)
def _mlp_problem(case):
    M, K, N, p = case
    g = torch.Generator().manual_seed(M + K)
    return dict(x=torch.randn(M, K, generator=g), gamma=1 + 0.3 * torch.randn(K, generator=g), beta=0.3 * torch.randn(K, generator=g),
                W=torch.randn(N, K, generator=g) / math.sqrt(K), b=0.3 * torch.randn(N, generator=g), gout=torch.randn(M, N, generator=g),
                keep=_keep(MLP_SEED, p, (M, K)))


def _mlp_restate(case, pr, dt, gate=None):
    """LN -> keep -> Linear (-> ReLU through ``gate``, the 0 / 1 derivative of the ReLU): pre-activations; with a gate the gradients"""
    M, K, N, p = case
    gamma, beta, W, b = (_leaf(pr[n], dt, gate is not None) for n in ("gamma", "beta", "W", "b"))
    z = F.layer_norm(pr["x"].to(dt), (K,), gamma, beta, EPS_LN) * pr["keep"].to(dt)
    pre = z @ W.t() + b
    out = dict(pre=pre.detach(), y=pre.detach().clamp(min=0))
    if gate is not None:
        (pre * (pr["gout"].to(dt) * gate.to(dt))).sum().backward()
        out.update(dgamma=gamma.grad, dbeta=beta.grad, dW=W.grad, db=b.grad)
    return out


def _mlp_band(pre64):
    """elements whose ReLU bit the test makes a claim about, and the share of the others"""
    claim = pre64.abs() >= BAND * pre64.abs().max()
    return claim, 1.0 - float(claim.double().mean())


@pytest.mark.gpu
@pytest.mark.parametrize("case", MLP_CASES, ids=_id)
def test_input_ln_linear_with_dropout_against_fp64(ops, case):
    M, K, N, p = case
    pr = _mlp_problem(case)
    xd = pr["x"].cuda()
    gd, bd, wd, cd = (_dev(pr[n], True) for n in ("gamma", "beta", "W", "b"))
    assert ops.input_ln_linear_supported(xd, wd)
    h = ops.input_ln_linear(xd, gd, bd, wd, cd, p=p, seed=MLP_SEED)
    h.backward(pr["gout"].cuda())
    torch.cuda.synchronize()
    pre = _mlp_restate(case, pr, torch.float64)["pre"]
    claim, share = _mlp_band(pre)
    assert share <= BAND_CAP, share
    on = (h.detach() > 0).cpu()
    assert torch.equal(on[claim], (pre > 0)[claim])                  # the ReLU bit wherever the reference is sure of it
    ref = _mlp_restate(case, pr, torch.float64, torch.where(claim, pre > 0, on))     # inside the band: the kernel's own bit
    got = dict(y=h.detach(), dgamma=gd.grad, dbeta=bd.grad, dW=wd.grad, db=cd.grad)
    for n in MLP_NAMES:
        _hold("input_ln_linear %s" % _id(case), n, got[n], ref[n], TOL, FACTOR * MLP_FP32)


# =====================================================================================================================
# Reference self-checks: no GPU.  The fp32 evaluation of each restatement against the fp64 one on the family's smallest case
# =====================================================================================================================
def _fp32_figure(family, case):
    """of-scale distance of the fp32 from the fp64 evaluation of a family's restatement on ``case``, worst tensor, on one thread; the
    rebuilt masks"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _fp32_figure_here(family, case)
    finally:
        torch.set_num_threads(threads)


def _fp32_figure_here(family, case):
    if family == "mha":
        pr = _mha_problem(case)
        return _worst(_mha_restate(case, pr, torch.float32), _mha_restate(case, pr, torch.float64), ("out", "dq", "dk", "dv")), [pr["keep"]]
    if family == "k1":
        pr = _k1_problem(case)
        return _worst(_k1_restate(pr, torch.float32), _k1_restate(pr, torch.float64), K1_NAMES), pr["keeps"]
    if family == "ln":
        pr = _ln_problem(case)
        return _worst(_ln_restate(case, pr, torch.float32), _ln_restate(case, pr, torch.float64), LN_NAMES), [pr["keep"]]
    if family == "cat3":
        pr = _cat3_problem(case)
        return _worst(_cat3_restate(case, pr, torch.float32), _cat3_restate(case, pr, torch.float64), CAT3_NAMES), [pr["keep"]]
    if family in ("lndw", "lndw_rows"):             # the row sums of the 12 000-row case have a constant of their own
        pr = _lndw_problem(case)
        M, L = case[:2]
        names = LNDW_ROW_SUMS if family == "lndw_rows" else [n for n in LNDW_NAMES if M * L <= 1000 or n not in LNDW_ROW_SUMS]
        return _worst(_lndw_restate(case, pr, torch.float32), _lndw_restate(case, pr, torch.float64), names), [pr["keep"]]
    if family == "l2":
        pr = _l2_problem(case)
        r32, r64 = _l2_restate(case, pr, torch.float32), _l2_restate(case, pr, torch.float64)
        e = max(_scale_err(r32[k], r64[k]) for k in ("y", "norm"))
        return max(e, _scale_err(_l2_live(r32["dx"]), _l2_live(r64["dx"]))), [pr["keep"]]
    assert family == "mlp"
    pr = _mlp_problem(case)
    pre = _mlp_restate(case, pr, torch.float64)["pre"]
    gate = pre > 0                                                   # one gate for both: the ReLU bit is not what this figure is about
    return _worst(_mlp_restate(case, pr, torch.float32, gate), _mlp_restate(case, pr, torch.float64, gate), MLP_NAMES), [pr["keep"]]


FP32_CHECKS = [("mha", MHA_MFMA[0], "MHA_FP32"), ("k1", K1_CASES[6], "K1_FP32"), ("ln", LN_CASES[0], "LN_FP32"), ("cat3", CAT3_CASES[0], "CAT3_FP32"),
               ("lndw", LNDW_CASES[9], "LNDW_FP32"), ("l2", L2_CASES[1], "L2_FP32"), ("mlp", MLP_CASES[3], "MLP_FP32")]


@pytest.mark.parametrize("family,case,const", FP32_CHECKS, ids=[c[0] for c in FP32_CHECKS])
def test_fp32_restatement_stays_inside_its_constant(family, case, const):
    """the constant a family's second bound is 16 x of: the fp32 CPU evaluation of its restatement is no further than that from the fp64
    one on the smallest case, and not zero (a restatement that ignores its dtype would make the bound empty); each rebuilt mask keeps
    1 - p of its elements to 5 sigma"""
    fig, keeps = _fp32_figure(family, case)
    print("    %-5s %-24s fp32 restatement of scale %.3e (%s = %.3e)" % (family, _id(case), fig, const, globals()[const]))
    assert 0.0 < fig <= globals()[const], (family, fig)
    _masks_ok(family, case, keeps)


def _masks_ok(family, case, keeps):
    p = K1_P if family == "k1" else CAT3_P if family == "cat3" else case[-1]
    for keep in keeps:
        ok, frac = _kept_ok(keep, p)
        assert ok, (family, frac, p)
        assert set(float(v) for v in keep.unique()) == {0.0, float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))}


# the case each constant was read off (and the 12 000-row ln_dwconv case once more for its other tensors)
FP32_WORST = [("mha", MHA_MFMA[6], "MHA_FP32"), ("k1", K1_CASES[8], "K1_FP32"), ("ln", LN_CASES[13], "LN_FP32"), ("cat3", CAT3_CASES[3], "CAT3_FP32"),
              ("lndw", LNDW_CASES[2], "LNDW_FP32"), ("lndw_rows", LNDW_CASES[6], "LNDW_ROWS_FP32"), ("l2", L2_CASES[5], "L2_FP32"),
              ("mlp", MLP_CASES[2], "MLP_FP32")]


@pytest.mark.parametrize("family,case,const", FP32_WORST, ids=[c[0] for c in FP32_WORST])
def test_fp32_constant_is_its_worst_case_rounded_up(family, case, const):
    """a constant is what its worst case gives, rounded up by less than a tenth: neither exceeded nor inflated"""
    fig, keeps = _fp32_figure(family, case)
    print("    %-9s %-24s fp32 restatement of scale %.3e (%s = %.3e)" % (family, _id(case), fig, const, globals()[const]))
    assert 0.9 * globals()[const] <= fig <= globals()[const], (family, fig)
    _masks_ok("lndw" if family == "lndw_rows" else family, case, keeps)


def test_ln_dwconv_row_case_keeps_the_small_constant_outside_its_row_sums():
    fig, _ = _fp32_figure("lndw", LNDW_CASES[6])
    assert 0.0 < fig <= LNDW_FP32, fig


def test_k1_reference_is_not_degenerate():
    """the K1 reference alone: A mostly non-zero, masked and unmasked score entries both present, every masked score -1e10 in fp32"""
    case = K1_CASES[6]
    pr = _k1_problem(case)
    with O.drop_masks(pr["keeps"]):
        A, S, Sm, Sn = O.structured_attention(pr["C"].double(), pr["Q"].double(), pr["cm"].double(), pr["qm"].double(), K1_SCALE, K1_P, True)
    assert float((A == 0).double().mean()) < 0.9
    assert 0.05 < float((Sm != 0).double().mean()) < 0.95
    assert bool((S[Sm == 0].float() == NEG32).all())


def test_input_mlp_relu_band_is_thin():
    """the ReLU band of case 7 on the reference alone: at most 1e-3 of the pre-activations lie within 1e-4 of scale of zero"""
    case = MLP_CASES[3]
    _, share = _mlp_band(_mlp_restate(case, _mlp_problem(case), torch.float64)["pre"])
    print("    input MLP %s: band share %.3e" % (_id(case), share))
    assert share <= BAND_CAP, share
