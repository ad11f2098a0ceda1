"""-m gpu: the first stage of the input MLP on half-precision feature rows (csrc/feat16.hip) -- [F.normalize] -> LayerNorm + dropout
read from fp16 / bf16 rows in place -- against an fp64 reference, measured side by side with the fp32 entry points on the upcast rows.

Bound (every output; both errors are measured in the run, nothing is fixed in advance):

    e_new <= 2 * e_old + 2^-22 * max|ref|

e_old = error of stage_l2norm[_gather]_fwd + stage_layernorm[_gather]_{fwd,bwd} on ``x.float()``, e_new = error of the new kernels on
``x``, both against torch's fp64 evaluation of the same formulas on ``x.double()`` (the conversion is exact, so all three see the same
numbers).  Both sides are fp32 evaluations of the same formulas that differ at most in summation order and contraction: a factor 2
and four units in the last place of the largest value cover that, while a wrong row, a wrong column or a wrong conversion is off by
orders of magnitude.  With dropout the reference carries the keep mask (the host restatement of csrc/common.h: drop4) and the
1 / (1 - p) factor, so the same bound holds on the scaled values.

x is a view into the middle of a buffer whose surroundings are NaN: a read outside the tensor that reaches a result shows as NaN.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DT = {"fp16": (torch.float16, 1), "bf16": (torch.bfloat16, 2)}
EPS_LN, EPS_L2 = 1e-5, 1e-12
P_DROP, SEED = 0.1, 0x5EED5EED1234
PAD = 64                      # halves of NaN in front of and behind x (128 bytes: x stays 8-byte aligned)
KS = [4, 12, 300, 768, 1024]  # one quad; quads < lanes of the smallest row group; 8-byte loads only; 3 quads per lane; the limit
MS = [1, 5, 67, 1031]         # one row; fewer rows than a wave iteration; several waves; several blocks + a ragged tail


def _keep(seed: int, p: float, n: int) -> np.ndarray:
    """keep flag of elements 0..n-1 of the dropout stream (csrc/common.h: mix64 + drop4, drop_thresh16)."""
    t = np.float32(p) * np.float32(65536.0) + np.float32(0.5)
    th = 0 if t <= 0 else (65535 if t >= 65535 else int(t))
    with np.errstate(over="ignore"):
        idx = np.arange((n + 3) // 4, dtype=np.uint64)
        z = np.uint64(seed) + (idx + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        h = z ^ (z >> np.uint64(31))
    f = np.stack([(h >> np.uint64(16 * i)) & np.uint64(0xFFFF) for i in range(4)], axis=1).reshape(-1)[:n]
    return f >= np.uint64(th)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Case:
    """Inputs of one grid point (host + device) and its fp64 references for p = 0 and p = P_DROP."""

    def __init__(self, dev, dtype_name, l2, gather, K0, M):
        tdt, self.code = DT[dtype_name]
        g = torch.Generator().manual_seed(1000 * K0 + 10 * M + 2 * l2 + gather + (5 if dtype_name == "bf16" else 0))
        R = 2 * M + 3 if gather else M
        if gather:
            if M == 1:
                src = torch.tensor([R - 1])                      # (a single row cannot hold both ends: the far one)
            else:
                mid = (torch.randperm(R - 2, generator=g)[: M - 2] + 1).sort().values
                src = torch.cat([torch.tensor([0]), mid, torch.tensor([R - 1])])
        else:
            src = torch.arange(M)
        x = (torch.randn(R, K0, generator=g) * 2.0 + 0.25).to(tdt)
        # rows the kernels must get right, among the rows that are read: all zero, the largest finite fp16 value, fp16 subnormals
        special = [torch.zeros(K0, dtype=tdt)]
        big = x[0].clone()
        big[K0 // 2] = 65504.0
        special.append(big)
        if tdt == torch.float16:
            k = torch.randint(-1023, 1024, (K0,), generator=g).to(torch.int16)
            special.append(((k.abs() & 0x3FF) | ((k < 0).to(torch.int16) << 15)).view(torch.float16))       # exponent field 0
        for i, row in enumerate(special):
            if i + 1 < M:
                x[src[i + 1]] = row
        buf = torch.full((R * K0 + 2 * PAD,), float("nan"), dtype=tdt)
        buf[PAD: PAD + R * K0] = x.reshape(-1)
        self.buf = buf.to(dev)
        self.x = self.buf[PAD: PAD + R * K0].view(R, K0)
        assert self.x.data_ptr() % 8 == 0
        self.x32 = self.x.float()                                # what the fp32 model made of such features on entry
        self.src = src.to(torch.int32).to(dev) if gather else None
        sign = lambda t: torch.where(torch.rand(t.shape, generator=g) < 0.5, -t, t)
        self.gamma = sign(torch.rand(K0, generator=g) + 0.5).to(dev)
        self.beta = sign(torch.rand(K0, generator=g) * 0.5 + 0.1).to(dev)
        self.dy = torch.randn(M, K0, generator=g).to(dev)
        self.l2, self.gather, self.K0, self.M, self.dev = l2, gather, K0, M, dev
        # fp64 reference on the host
        xd = x.double()[src]
        if l2:
            xd = F.normalize(xd, dim=-1, eps=EPS_L2)
        mean = xd.mean(-1)
        var = xd.var(-1, unbiased=False)
        rstd = 1.0 / torch.sqrt(var + EPS_LN)
        xh = (xd - mean[:, None]) * rstd[:, None]
        y = F.layer_norm(xd, (K0,), self.gamma.cpu().double(), self.beta.cpu().double(), EPS_LN)
        self.ref = {}
        for p in (0.0, P_DROP):
            if p > 0:
                inv_keep = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
                keep = torch.from_numpy(_keep(SEED, p, M * K0).reshape(M, K0))
                m = keep.double() * inv_keep
            else:
                keep, m = torch.ones(M, K0, dtype=torch.bool), torch.ones(M, K0, dtype=torch.float64)
            dyd = self.dy.cpu().double() * m
            self.ref[p] = dict(y0=y * m, mean0=mean, rstd0=rstd, dgamma=(dyd * xh).sum(0), dbeta=dyd.sum(0), keep=keep)

    def _outs(self):
        M, K0, dev = self.M, self.K0, self.dev
        nan = lambda *s: torch.full(s, float("nan"), device=dev)
        return dict(y0=nan(M, K0), mean0=nan(M), rstd0=nan(M), dgamma=nan(K0), dbeta=nan(K0))

    def run_old(self, lib, p):
        """the fp32 entry points on the upcast rows, called as csrc/groups.hip (input_mlp_fwd / input_mlp_bwd) calls them"""
        from tvqaplus_amd import _lib
        o, M, K0 = self._outs(), self.M, self.K0
        seed = SEED if p > 0 else 0
        xin, gat = self.x32, self.src
        if self.l2:
            xn = torch.empty(M, K0, device=self.dev)
            if gat is not None:
                _lib.check(lib.stage_l2norm_gather_fwd(xin.data_ptr(), gat.data_ptr(), xn.data_ptr(), M, K0, EPS_L2, _stream()), "l2 gather")
            else:
                _lib.check(lib.stage_l2norm_fwd(xin.data_ptr(), xn.data_ptr(), None, M, K0, EPS_L2, 0.0, 0, _stream()), "l2")
            xin, gat = xn, None
        ws_b = lib.stage_ln_bwd_ws_bytes(K0)
        ws = torch.empty(ws_b, dtype=torch.uint8, device=self.dev)
        if gat is not None:
            _lib.check(lib.stage_layernorm_gather_fwd(xin.data_ptr(), gat.data_ptr(), self.gamma.data_ptr(), self.beta.data_ptr(),
                                                      o["y0"].data_ptr(), o["mean0"].data_ptr(), o["rstd0"].data_ptr(), M, K0, EPS_LN, p, seed,
                                                      _stream()), "ln gather fwd")
            _lib.check(lib.stage_layernorm_gather_bwd(self.dy.data_ptr(), xin.data_ptr(), gat.data_ptr(), o["mean0"].data_ptr(),
                                                      o["rstd0"].data_ptr(), self.gamma.data_ptr(), o["dgamma"].data_ptr(), o["dbeta"].data_ptr(),
                                                      M, K0, p, seed, ws.data_ptr(), ws_b, _stream()), "ln gather bwd")
        else:
            _lib.check(lib.stage_layernorm_fwd(xin.data_ptr(), None, 0, None, self.gamma.data_ptr(), self.beta.data_ptr(), o["y0"].data_ptr(),
                                               o["mean0"].data_ptr(), o["rstd0"].data_ptr(), M, K0, EPS_LN, p, seed, _stream()), "ln fwd")
            _lib.check(lib.stage_layernorm_bwd(self.dy.data_ptr(), xin.data_ptr(), o["mean0"].data_ptr(), o["rstd0"].data_ptr(),
                                               self.gamma.data_ptr(), None, None, o["dgamma"].data_ptr(), o["dbeta"].data_ptr(), M, K0, p, seed,
                                               ws.data_ptr(), ws_b, _stream()), "ln bwd")
        torch.cuda.synchronize()
        return o

    def run_new(self, lib, p):
        from tvqaplus_amd import _lib
        o, M, K0 = self._outs(), self.M, self.K0
        seed = SEED if p > 0 else 0
        gat = None if self.src is None else self.src.data_ptr()
        ws_b = lib.stage_feat16_ln_bwd_ws_bytes(K0)
        ws = torch.empty(ws_b, dtype=torch.uint8, device=self.dev)
        _lib.check(lib.stage_feat16_ln_fwd(self.x.data_ptr(), self.code, gat, self.gamma.data_ptr(), self.beta.data_ptr(), o["y0"].data_ptr(),
                                           o["mean0"].data_ptr(), o["rstd0"].data_ptr(), M, K0, int(self.l2), EPS_LN, EPS_L2, p, seed,
                                           _stream()), "stage_feat16_ln_fwd")
        _lib.check(lib.stage_feat16_ln_bwd(self.dy.data_ptr(), self.x.data_ptr(), self.code, gat, o["mean0"].data_ptr(), o["rstd0"].data_ptr(),
                                           o["dgamma"].data_ptr(), o["dbeta"].data_ptr(), M, K0, int(self.l2), EPS_L2, p, seed, ws.data_ptr(),
                                           ws_b, _stream()), "stage_feat16_ln_bwd")
        torch.cuda.synchronize()
        return o


def _err(got, ref):
    d = (got.detach().double().cpu() - ref).abs()
    return float("inf") if bool(torch.isnan(d).any()) else float(d.max())


@pytest.fixture(scope="module")
def lib(hip_device):
    from tvqaplus_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K0", KS)
@pytest.mark.parametrize("gather", [0, 1], ids=["rows", "table"])
@pytest.mark.parametrize("l2", [0, 1], ids=["ln", "l2ln"])
@pytest.mark.parametrize("dtype_name", ["fp16", "bf16"])
def test_first_stage_vs_fp64_and_the_fp32_path(hip_device, lib, dtype_name, l2, gather, K0, M):
    c = Case(hip_device, dtype_name, l2, gather, K0, M)
    for p in (0.0, P_DROP):
        ref = c.ref[p]
        old, new, again = c.run_old(lib, p), c.run_new(lib, p), c.run_new(lib, p)
        for k in ("y0", "mean0", "rstd0", "dgamma", "dbeta"):
            assert torch.equal(new[k], again[k]), (k, "two runs differ")
            assert bool(torch.isfinite(new[k]).all()), (k, "not finite: a read outside the tensor, or an unwritten element")
            e_old, e_new = _err(old[k], ref[k]), _err(new[k], ref[k])
            bound = 2.0 * e_old + 2.0 ** -22 * float(ref[k].abs().max())
            print("%s l2=%d gather=%d K0=%d M=%d p=%.1f %-6s e_old %.3e e_new %.3e bound %.3e" % (dtype_name, l2, gather, K0, M, p, k,
                                                                                                 e_old, e_new, bound))
            assert e_new <= bound, (k, p, e_old, e_new, bound)
        if p > 0:
            # the dropout stream of the fp32 path: the same elements dropped, and they are the ones the host restatement names
            zero_new, zero_old = new["y0"] == 0, old["y0"] == 0
            assert torch.equal(zero_new, zero_old)
            assert torch.equal(zero_new.cpu(), ~ref["keep"])


def test_unsupported_arguments_are_refused_before_a_launch(hip_device, lib):
    from tvqaplus_amd import _lib
    dev = hip_device
    M, K0 = 5, 1028
    buf = torch.ones(M * K0 + 8, dtype=torch.float16, device=dev)
    gamma, beta = torch.ones(K0, device=dev), torch.zeros(K0, device=dev)
    ws = torch.empty(lib.stage_ln_bwd_ws_bytes(1024) * 2, dtype=torch.uint8, device=dev)
    cases = [(6, 1, 0), (1028, 1, 0), (1028, 2, 0), (768, 0, 0), (768, 3, 0), (300, 1, 1), (768, 2, 3), (0, 1, 0)]   # K0, dtype code, element offset
    for k0, code, off in cases:
        y = torch.full((M, K0), -7.0, device=dev)
        mean, rstd = torch.full((M,), -7.0, device=dev), torch.full((M,), -7.0, device=dev)
        dg, db = torch.full((K0,), -7.0, device=dev), torch.full((K0,), -7.0, device=dev)
        x = buf[off:]
        assert (x.data_ptr() % 8 != 0) == (off % 4 != 0)
        rc = lib.stage_feat16_ln_fwd(x.data_ptr(), code, None, gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                     M, k0, 1, EPS_LN, EPS_L2, 0.1, 3, _stream())
        assert rc == _lib.STAGE_ERR_SHAPE, (k0, code, off, rc)
        rc = lib.stage_feat16_ln_bwd(y.data_ptr(), x.data_ptr(), code, None, mean.data_ptr(), rstd.data_ptr(), dg.data_ptr(), db.data_ptr(), M, k0,
                                     1, EPS_L2, 0.1, 3, ws.data_ptr(), ws.numel(), _stream())
        assert rc == _lib.STAGE_ERR_SHAPE, (k0, code, off, rc)
        torch.cuda.synchronize()
        for t in (y, mean, rstd, dg, db):
            assert bool((t == -7.0).all()), (k0, code, off, "something was written")
    # a workspace smaller than the query names: refused as such
    y = torch.zeros(M, 768, device=dev)
    st = torch.zeros(M, device=dev)
    dg = torch.full((768,), -7.0, device=dev)
    rc = lib.stage_feat16_ln_bwd(y.data_ptr(), buf.data_ptr(), 1, None, st.data_ptr(), st.data_ptr(), dg.data_ptr(), dg.data_ptr(), M, 768, 0,
                                 EPS_L2, 0.0, 0, ws.data_ptr(), lib.stage_feat16_ln_bwd_ws_bytes(768) - 1, _stream())
    assert rc == _lib.STAGE_ERR_WORKSPACE
    # the group entry points refuse the same arguments (the caller then upcasts and runs the fp32 group)
    from tvqaplus_amd import groups
    assert groups.feat16_ok(buf[: M * 768].view(M, 768)) and groups.feat16_ok(buf[: M * 768].view(M, 768).bfloat16())
    assert not groups.feat16_ok(buf[1: 1 + M * 768].view(M, 768))               # 2 bytes into the buffer
    assert not groups.feat16_ok(buf[: M * 1028].view(M, 1028))                  # wider than the row kernels take
    assert not groups.feat16_ok(buf[: M * 768].view(M, 768)[:, :300])           # rows not contiguous
    assert not groups.feat16_ok(buf[: M * 6].view(M, 6))
    assert not groups.feat16_ok(buf[: M * 768].view(M, 768).float())
    params = [torch.ones(8, device=dev) for _ in range(10)]
    with pytest.raises(groups.Unsupported):
        groups.input_mlp(buf[1: 1 + M * 768].view(M, 768), False, 0.0, (0, 0), params)
