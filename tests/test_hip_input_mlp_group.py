"""-m gpu: the input-MLP group (G1: csrc/groups.hip, stage_grp_input_mlp_{fwd,bwd}) in every form of its first stage -- fp32 / fp16 /
bf16 rows x every row / the rows a table names x with / without F.normalize x dropout off / on -- against the same chain spelled out
as per-kernel calls: the first stage as tests/test_hip_feat16.py::Case spells it (run_old: the fp32 entry points, run_new: the
half-precision ones), the tail through the tvqaplus_amd.ops wrappers of STAGE.base_encoder's per-op branch.  The group only sequences
those kernels, with the same arguments and workspace sizes, so ``out`` and the ten parameter gradients are held to torch.equal.

x is a view into the middle of a buffer whose surroundings are NaN; the table has gaps and names the first and the last source row.
"""
import ctypes
import types

import pytest
import torch

from test_hip_feat16 import PAD, P_DROP, SEED, Case

pytestmark = pytest.mark.gpu

SEED1 = 0x1234ABCD5EED
M_MASK = 4096                 # the smallest M at which stage_gemm_mask_supported(M, 64, 64) answers 1 (test_mask_shape_is_the_threshold)
SHAPES = [(5, 12, 8, 8),                    # fewer rows than a wave iteration; tiled GEMMs
          (1031, 300, 300, 128),            # several blocks and a row tail on the tiled GEMMs
          (M_MASK + 77, 64, 64, 64)]        # both Linear + ReLU layers on the streaming kernels with the ReLU bit mask, a 77-row tail
DTYPES = ["fp32", "fp16", "bf16"]


@pytest.fixture(scope="module")
def lib(hip_device):
    from tvqaplus_amd import _lib
    return _lib.load()


def test_mask_shape_is_the_threshold(lib):
    _, K0, H, D = SHAPES[2]
    assert lib.stage_gemm_mask_supported(M_MASK, H, K0) == 1 and lib.stage_gemm_mask_supported(M_MASK, D, H) == 1
    assert lib.stage_gemm_mask_supported(M_MASK - 1, H, K0) == 0 and lib.stage_gemm_mask_supported(M_MASK - 1, D, H) == 0
    for M, K0, H, D in SHAPES[:2]:
        assert lib.stage_gemm_mask_supported(M, H, K0) == 0 and lib.stage_gemm_mask_supported(M, D, H) == 0


class Form:
    """One grid point: Case's features (fp32 form: its upcast rows, moved into a NaN-padded buffer of their own), the MLP's
    parameters behind the first LayerNorm, the output gradient."""

    def __init__(self, dev, dtype_name, table, l2, shape):
        M, K0, H, D = shape
        self.c = c = Case(dev, "fp16" if dtype_name == "fp32" else dtype_name, l2, table, K0, M)
        self.fp32 = dtype_name == "fp32"
        if self.fp32:
            R = c.x.shape[0]
            buf = torch.full((R * K0 + 2 * PAD,), float("nan"), device=dev)
            buf[PAD: PAD + R * K0] = c.x32.reshape(-1)
            c.x32 = buf[PAD: PAD + R * K0].view(R, K0)
        self.x = c.x32 if self.fp32 else c.x
        g = torch.Generator().manual_seed(7 * M + K0 + H + D)
        r = lambda *s: torch.randn(*s, generator=g)
        tail = [r(H, K0) / K0 ** 0.5, 0.1 * r(H), 1 + 0.2 * r(H), 0.1 * r(H), r(D, H) / H ** 0.5, 0.1 * r(D), 1 + 0.2 * r(D), 0.1 * r(D)]
        self.params = [c.gamma, c.beta] + [t.to(dev) for t in tail]
        self.dout = r(M, D).to(dev)
        self.clay = types.SimpleNamespace(U=M, Ucap=M + 3, src_rows=c.src) if table else None
        self.l2, self.shape = l2, shape

    def group(self, p):
        from tvqaplus_amd import groups
        ps = [w.detach().clone().requires_grad_(True) for w in self.params]
        seeds = (SEED, SEED1) if p > 0 else (0, 0)
        if self.clay is None:
            out = groups.input_mlp(self.x, self.l2, p, seeds, ps)
        else:
            out = groups.input_mlp_rag(self.x, self.clay, self.l2, p, seeds, ps)
        grads = torch.autograd.grad(out, ps, self.dout)
        torch.cuda.synchronize()
        return out.detach(), grads

    def chain(self, lib, p):
        from tvqaplus_amd import ops
        c = self.c
        first = c.run_old if self.fp32 else c.run_new
        y0 = first(lib, p)["y0"].requires_grad_(True)             # (its gradients: of Case's own dy, not wanted yet)
        ps = [w.detach().clone().requires_grad_(True) for w in self.params[2:]]
        h1 = ops.linear(y0, ps[0], ps[1], relu=True)
        y1, _ = ops.layernorm(h1, ps[2], ps[3], p=p, seed=SEED1 if p > 0 else 0)
        h2 = ops.linear(y1, ps[4], ps[5], relu=True)
        out, _ = ops.layernorm(h2, ps[6], ps[7])
        dy0, *gtail = torch.autograd.grad(out, [y0] + ps, self.dout)
        c.dy = dy0.contiguous()
        o = first(lib, p)
        return out.detach(), [o["dgamma"], o["dbeta"]] + gtail


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("l2", [0, 1], ids=["ln", "l2ln"])
@pytest.mark.parametrize("table", [0, 1], ids=["rows", "table"])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_every_form_equals_the_spelled_out_chain(hip_device, lib, dtype_name, table, l2, shape):
    f = Form(hip_device, dtype_name, table, l2, shape)
    for p in (0.0, P_DROP):
        ref_out, ref_g = f.chain(lib, p)
        out, g = f.group(p)
        out2, g2 = f.group(p)
        assert out.shape == ref_out.shape and bool(torch.isfinite(out).all())
        d = [float((a.reshape(-1) - b.reshape(-1)).abs().max()) for a, b in zip([out] + list(g), [ref_out] + ref_g)]
        print("%s table=%d l2=%d %s p=%.1f max|group - chain|: out %.3e grads %s" % (dtype_name, table, l2, shape, p, d[0],
                                                                                  " ".join("%.3e" % v for v in d[1:])))
        assert torch.equal(out, ref_out), (p, d[0])
        assert torch.equal(out, out2), (p, "two runs differ")
        for i, (a, b, a2) in enumerate(zip(g, ref_g, g2)):
            assert torch.equal(a.reshape(-1), b.reshape(-1)), (p, i, d[1 + i])
            assert torch.equal(a, a2), (p, i, "two runs differ")


def test_refusals_come_before_a_launch(hip_device, lib):
    from tvqaplus_amd import _lib
    dev = hip_device
    M, W = 5, 1028                                     # every buffer is sized for W-wide layers: a call that was not refused stays inside
    stream = torch.cuda.current_stream().cuda_stream
    xbuf = torch.ones(M * W * 2 + 8, dtype=torch.float16, device=dev)           # (also M * W floats)
    params = [torch.ones(W * W if i in (2, 6) else W, device=dev) for i in range(10)]
    ptrs = lambda ts: (ctypes.c_void_p * 10)(*[t.data_ptr() for t in ts])
    seeds = (ctypes.c_ulonglong * 2)(3, 4)
    big = int(lib.stage_grp_input_mlp_arena_bytes(M, W, W, W, 1, 0))
    tmp_b = int(lib.stage_grp_input_mlp_bwd_tmp_bytes(M, W, W, W))

    def call(dtype, off, m, K0, H, D, arena_bytes=None, tmp_bytes=None, bwd=False):
        out = torch.full((M, W), -7.0, device=dev)
        arena = torch.full((big,), 0x5A, dtype=torch.uint8, device=dev)
        tmp = torch.full((tmp_b,), 0x5A, dtype=torch.uint8, device=dev)
        grads = [torch.full_like(w, -7.0) for w in params]
        flags = (ctypes.c_int * 16)()
        x = xbuf[off:]
        ab = big if arena_bytes is None else arena_bytes
        rc = lib.stage_grp_input_mlp_fwd(x.data_ptr(), dtype, None, ptrs(params), out.data_ptr(), arena.data_ptr(), ab, flags, m, K0, H, D,
                                         1, 0.1, seeds, stream)
        rcs = [rc]
        if bwd:
            rcs.append(lib.stage_grp_input_mlp_bwd(out.data_ptr(), x.data_ptr(), dtype, None, ptrs(params), ptrs(grads), arena.data_ptr(),
                                                   ab, flags, tmp.data_ptr(), tmp_b if tmp_bytes is None else tmp_bytes, m, K0, H, D, 1,
                                                   0.1, seeds, stream))
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((arena == 0x5A).all()) and bool((tmp == 0x5A).all()), "something was written"
        assert all(bool((t == -7.0).all()) for t in grads), "something was written"
        return rcs

    F32, F16 = _lib.STAGE_DT_F32, _lib.STAGE_DT_F16
    assert call(3, 0, M, 8, 8, 8, bwd=True) == [_lib.STAGE_ERR_SHAPE] * 2                 # no such dtype
    assert xbuf[1:].data_ptr() % 8 == 2
    assert call(F16, 1, M, 8, 8, 8, bwd=True) == [_lib.STAGE_ERR_SHAPE] * 2               # half rows two bytes off alignment
    assert call(F32, 0, M, 6, 8, 8) == [_lib.STAGE_ERR_SHAPE]
    assert call(F32, 0, M, 8, 6, 8) == [_lib.STAGE_ERR_SHAPE]
    assert call(F16, 0, M, 8, 6, 8, bwd=True) == [_lib.STAGE_ERR_SHAPE] * 2
    assert call(F32, 0, 0, 8, 8, 8) == [_lib.STAGE_ERR_SHAPE]
    assert call(F16, 0, 0, 8, 8, 8, bwd=True) == [_lib.STAGE_ERR_SHAPE] * 2
    assert call(F16, 0, M, 1028, 8, 8, bwd=True) == [_lib.STAGE_ERR_SHAPE] * 2            # wider than the half-precision row kernels take
    # a buffer one byte below what the query names: refused as such, in both directions
    for dtype in (F32, F16):
        need = int(lib.stage_grp_input_mlp_arena_bytes(M, 8, 8, 8, 1, dtype))
        assert call(dtype, 0, M, 8, 8, 8, arena_bytes=need - 1, bwd=True) == [_lib.STAGE_ERR_WORKSPACE] * 2
        tneed = int(lib.stage_grp_input_mlp_bwd_tmp_bytes(M, 8, 8, 8))
        out = torch.full((M, 8), -7.0, device=dev)
        grads = [torch.full_like(w, -7.0) for w in params]
        arena = torch.zeros(big, dtype=torch.uint8, device=dev)
        tmp = torch.full((tmp_b,), 0x5A, dtype=torch.uint8, device=dev)
        rc = lib.stage_grp_input_mlp_bwd(out.data_ptr(), xbuf.data_ptr(), dtype, None, ptrs(params), ptrs(grads), arena.data_ptr(), need,
                                         (ctypes.c_int * 16)(), tmp.data_ptr(), tneed - 1, M, 8, 8, 8, 1, 0.1, seeds, stream)
        torch.cuda.synchronize()
        assert rc == _lib.STAGE_ERR_WORKSPACE
        assert bool((tmp == 0x5A).all()) and all(bool((t == -7.0).all()) for t in grads)
