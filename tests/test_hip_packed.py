"""-m gpu: packed context features on the device (csrc/packed.hip, tvqaplus_amd/packed.py, ragged.CtxLayout(packed=...), STAGE).

The two kernels are held to their host specifications byte for byte (``PackedFeatures.unpad_host``, ``CtxTables.src_rows_packed_host``);
the whole model on a packed batch is held to the same model on the padded batch BIT FOR BIT: it reads the same numbers through the same
kernels in the same order, so nothing may differ -- after the precondition that two padded runs do not differ either."""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GUARD = 3                   # guard rows in front of and behind every buffer
LENS7 = [0, 5, 1, 3, 0, 5, 2]
DT = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}


def _bytes(t):
    return t.contiguous().view(torch.uint8).reshape(-1)


def _packed_case(lens, L, K, dtype, seed=0):
    from tvqaplus_amd.packed import PackedFeatures
    lens = np.asarray(lens, dtype=np.int32).reshape(1, -1)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, lens.shape[1], L, K, generator=g)
    x = x * (torch.arange(L).view(1, 1, L) < torch.from_numpy(lens.astype(np.int64)).unsqueeze(-1)).unsqueeze(-1)
    return PackedFeatures.from_padded(x.to(dtype), lens, check=True)


def _aligned(nbytes, fill, dev, shift):
    """A device byte buffer of ``nbytes`` filled with ``fill`` whose base is ``shift`` bytes behind a 16-byte boundary."""
    raw = torch.full((nbytes + 32,), fill, dtype=torch.uint8, device=dev)
    o = (shift - raw.data_ptr()) % 16
    return raw[o:o + nbytes]


def _unpack(lib, dev, pf, shift=0, with_mask=True):
    """stage_pack_unpack on guarded, pre-filled buffers -> (dense bytes, mask) after checking that no guard byte changed."""
    from tvqaplus_amd.ops import _stream
    frames, L, rb = pf.N * pf.Li, pf.L, pf.K * pf.data.element_size()
    g = GUARD * rb
    pbuf = _aligned(2 * g + pf.nbytes, 0xA5, dev, shift)
    pbuf[g:g + pf.nbytes] = _bytes(pf.data).to(dev)
    dbuf = _aligned(2 * g + frames * L * rb, 0xFF, dev, 0)                      # 0xFF..: NaN in every float format
    mbuf = torch.full((2 * GUARD + frames * L,), float("nan"), device=dev)
    ptab = torch.from_numpy(pf.ptab().reshape(-1)).to(dev)
    before = pbuf.clone()
    rc = lib.stage_pack_unpack(pbuf[g:].data_ptr(), ptab.data_ptr(), dbuf[g:].data_ptr(), mbuf[GUARD:].data_ptr() if with_mask else None,
                               frames, L, rb, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert torch.equal(pbuf, before)                                            # the source is only read
    assert bool((dbuf[:g] == 0xFF).all()) and bool((dbuf[g + frames * L * rb:] == 0xFF).all()), "dense guard rows were written"
    assert bool(torch.isnan(mbuf[:GUARD]).all()) and bool(torch.isnan(mbuf[GUARD + frames * L:]).all()), "mask guards were written"
    return dbuf[g:g + frames * L * rb].cpu(), mbuf[GUARD:GUARD + frames * L].cpu()


@pytest.fixture(scope="module")
def lib():
    from tvqaplus_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("K,dt,shift", [(4, "fp16", 0), (300, "fp16", 0), (300, "fp32", 0), (768, "bf16", 0), (768, "fp32", 0),
                                        (1024, "fp32", 0), (300, "fp32", 8), (1024, "fp32", 8)])
def test_unpack_equals_the_host_specification_byte_for_byte(hip_device, lib, K, dt, shift):
    """Row bytes 8 (one chunk), 600 (rows alternate between 16- and 8-byte alignment: the 8-byte path), 1200 (16-byte path), 1536,
    3072, 4096 (the widest row); shift 8: 16-byte rows on a packed base that is only 8-byte aligned (8-byte path; 4096-byte rows then take eight chunks per lane)."""
    from tvqaplus_amd.ops import _stream
    pf = _packed_case(LENS7, 5, K, DT[dt], seed=K)
    assert pf.K * pf.data.element_size() == {(4, "fp16"): 8, (300, "fp16"): 600, (300, "fp32"): 1200, (768, "bf16"): 1536,
                                             (768, "fp32"): 3072, (1024, "fp32"): 4096}[(K, dt)]
    want, want_mask = pf.unpad_host()
    dense, mask = _unpack(lib, hip_device, pf, shift=shift)
    assert torch.equal(dense, _bytes(want))
    assert torch.equal(mask, want_mask.reshape(-1))
    dense2, mask2 = _unpack(lib, hip_device, pf, shift=shift, with_mask=False)
    assert torch.equal(dense2, _bytes(want)) and bool(torch.isnan(mask2).all())             # mask == NULL: no mask is written
    # the mask-only call: packed == dense == NULL
    mbuf = torch.full((2 * GUARD + 7 * 5,), float("nan"), device=hip_device)
    ptab = torch.from_numpy(pf.ptab().reshape(-1)).to(hip_device)
    assert lib.stage_pack_unpack(None, ptab.data_ptr(), None, mbuf[GUARD:].data_ptr(), 7, 5, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(mbuf[GUARD:GUARD + 35].cpu(), want_mask.reshape(-1))
    assert bool(torch.isnan(mbuf[:GUARD]).all()) and bool(torch.isnan(mbuf[GUARD + 35:]).all())


def test_unpack_more_rows_than_the_grid_holds(hip_device, lib):
    """84 000 rows of 600 bytes: more row groups than the capped grid has workgroups, so every workgroup walks several."""
    g = torch.Generator().manual_seed(9)
    lens = torch.randint(0, 21, (4200,), generator=g).tolist()
    lens[0], lens[1], lens[-1] = 20, 0, 20
    pf = _packed_case(lens, 20, 300, torch.float16, seed=10)
    want, want_mask = pf.unpad_host()
    dense, mask = _unpack(lib, hip_device, pf)
    assert torch.equal(dense, _bytes(want)) and torch.equal(mask, want_mask.reshape(-1))


@pytest.mark.parametrize("halo", [6, 1 << 20])
def test_packed_source_rows_on_the_device_equal_the_host_restatement(hip_device, lib, halo):
    from tvqaplus_amd import ragged
    from tvqaplus_amd.ops import _stream
    from tvqaplus_amd.packed import PackedFeatures
    L = 8
    lens = np.array([[0, 8, 5], [1, 2, 0], [8, 3, 7]], dtype=np.int32)         # len = 0, len = L, len + 6 > L
    x = torch.randn(3, 3, L, 12) * (torch.arange(L).view(1, 1, L) < torch.from_numpy(lens.astype(np.int64)).unsqueeze(-1)).unsqueeze(-1)
    pf = PackedFeatures.from_padded(x, lens, check=True).to(hip_device)
    ct = ragged.CtxTables(lens, L, halo)
    cl = ragged.CtxLayout(ct, hip_device, packed=pf)
    want = ct.src_rows_packed_host(pf.ptab(), pf.P)
    assert ct.U == int(np.where(lens > 0, np.minimum(L, lens + halo), 0).sum())
    src = torch.full((ct.U + 8,), -7, dtype=torch.int32, device=hip_device)
    assert lib.stage_pack_ctx_rows(cl.cq.data_ptr(), cl.ptab.data_ptr(), 9, L, pf.P, src.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(src[:ct.U].cpu().numpy(), want) and bool((src[ct.U:] == -7).all())
    assert np.array_equal(cl.src_rows[:ct.U].cpu().numpy(), want)              # what the layout itself launched
    # ... and the rows it names hold what the padded table's rows hold
    assert torch.equal(pf.data[cl.src_rows[:ct.U].long()].cpu(), x.view(-1, 12)[torch.from_numpy(ct.src_rows_host()).long()])
    assert torch.equal(cl.prefix_mask().cpu(), pf.unpad_host()[1])


# ---- whole model ----------------------------------------------------------------------------------------------------------------
SHAPE = dict(N=2, Li=6, Lr=8, Lw=10, Lqa=12, wd_size=96, vfeat_size=64)
MODEL_CFGS = {
    "default": dict(),
    "no_ragged": dict(_use_ragged=False),
    "heads2": dict(input_encoder_n_heads=2),
    "bf16_storage": dict(storage_dtype="bf16"),
    "fp16_features": dict(_half=True),
    "sub_only": dict(vfeat_flag=False),
    "vid_only": dict(sub_flag=False),
    "empty_frames": dict(_empty=True),
}


def _model(cfg, device):
    from tvqaplus_amd.stage import STAGE
    from tvqaplus_amd.synth import make_opt
    kw = {k: v for k, v in cfg.items() if not k.startswith("_")}
    torch.manual_seed(21)
    with contextlib.redirect_stdout(io.StringIO()):
        model = STAGE(make_opt(hsz=128, embedding_size=96, vfeat_size=64, dropout=0.1, add_local=True, **kw))
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.05 * torch.randn_like(p))
    model = model.to(device)
    model.use_ragged = cfg.get("_use_ragged", True)
    return model


def _batches(cfg, device):
    from tvqaplus_amd.synth import make_batch
    kw = dict(SHAPE, seed=17, empty_frames=bool(cfg.get("_empty")))
    pad, pk = make_batch(**kw), make_batch(packed=True, **kw)
    if cfg.get("_half"):
        pad.sub_bert, pad.vid = pad.sub_bert.to(torch.float16), pad.vid.to(torch.float16)
        pk.sub_bert, pk.vid = pk.sub_bert.to(torch.float16), pk.vid.to(torch.float16)
    return pad.to(device), pk.to(device)


def _train(model, batch):
    model.train()
    model._seed_state = 12345
    torch.manual_seed(99)
    for p in model.parameters():
        p.grad = None
    (out, targets), att_loss, _, t_loss, t_scores, other = model.forward_main(batch)
    loss = F.cross_entropy(out, targets, reduction="sum") * (len(batch.qid) / len(targets)) + 0.5 * t_loss
    loss.backward()
    torch.cuda.synchronize()
    res = {"logits": out.detach().clone(), "targets": targets.clone(), "t_scores": t_scores.detach().clone(), "t_loss": t_loss.detach().clone(),
           "loss": loss.detach().clone()}
    res.update({k: v.detach().clone() for k, v in other.items()})
    res.update({"grad/" + k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()})
    return res


def _eval(model, batch):
    model.eval()
    with torch.no_grad():
        out, _, _, t_loss, t_prob, other = model.forward_main(batch)
    torch.cuda.synchronize()
    res = {"logits": out.clone(), "t_scores": t_prob.clone(), "t_loss": t_loss.clone()}
    res.update({k: v.clone() for k, v in other.items()})
    return res


def _differing(a, b):
    assert set(a) == set(b)
    return sorted(k for k in a if not torch.equal(a[k], b[k]))


@pytest.mark.parametrize("name", list(MODEL_CFGS))
def test_model_on_a_packed_batch_equals_the_padded_batch_bit_for_bit(hip_device, name):
    """One training step (dropout 0.1) and one eval forward, same weights, same seeds.  Precondition: two runs on the PADDED batch
    agree bit for bit in every compared tensor (logits, temporal scores, every score map, the losses, every parameter gradient); then
    the packed batch must give the same bits.  No tensor is exempt."""
    cfg = MODEL_CFGS[name]
    model = _model(cfg, hip_device)
    pad, pk = _batches(cfg, hip_device)
    for run in (_train, _eval):
        a, b = run(model, pad), run(model, pad)
        lay_pad = (model.last_ragged is not None, sorted(model.last_ragged_ctx))
        p = run(model, pk)
        lay_pk = (model.last_ragged is not None, sorted(model.last_ragged_ctx))
        pre, diff = _differing(a, b), _differing(a, p)
        print("%s %s: layouts %r, %d tensors, padded-vs-padded differ %r, packed-vs-padded differ %r"
              % (name, run.__name__, lay_pk, len(a), pre, diff))
        assert lay_pad == lay_pk, "the packed batch took another path than the padded batch"
        streams = (["sub"] if model.sub_flag else []) + (["vid"] if model.vfeat_flag else [])
        if name in ("default", "heads2", "fp16_features", "sub_only", "vid_only", "empty_frames"):
            assert lay_pk == (True, streams), "the ragged context layout did not take the packed streams"
        else:
            assert lay_pk[1] == [], "this configuration is meant to unpack"
        assert not pre, "precondition: two padded runs differ in %r" % pre
        assert not diff, diff
        assert all(bool(torch.isfinite(v).all()) for k, v in p.items() if k.startswith("grad/") or k in ("logits", "loss", "t_loss"))


def test_packed_step_makes_no_more_library_calls_than_the_padded_step_plus_its_masks(hip_device):
    """Host issue time is the scarce resource: on the default path the packed step makes at most the padded step's C calls plus one
    mask call per context stream, and never builds a dense image."""
    import tvqaplus_amd._lib as L
    from tvqaplus_amd import ops
    lib = L.load()
    model = _model({}, hip_device)
    pad, pk = _batches({}, hip_device)

    def run(batch):
        seen, unpack_args = {}, []
        names = [k for k in L.SIGNATURES if not k.endswith("_bytes") and "supported" not in k and "recomputes" not in k
                 and k not in ("stage_hip_abi_version", "stage_hip_error_string")]
        real = {k: getattr(lib, k) for k in names}
        for k in names:
            def wrap(*a, _f=real[k], _k=k):
                seen[_k] = seen.get(_k, 0) + 1
                if _k == "stage_pack_unpack":
                    unpack_args.append(a)
                return _f(*a)
            setattr(lib, k, wrap)
        ops._FN.clear()
        try:
            _train(model, batch)
        finally:
            for k in names:
                setattr(lib, k, real[k])
            ops._FN.clear()
        return seen, unpack_args
    run(pad), run(pk)                                             # anything set up lazily happens here
    (c_pad, u_pad), (c_pk, u_pk) = run(pad), run(pk)
    print("library calls per training step: padded %d, packed %d; packed-only %r" % (
        sum(c_pad.values()), sum(c_pk.values()), {k: v for k, v in c_pk.items() if v != c_pad.get(k, 0)}))
    assert sorted(model.last_ragged_ctx) == ["sub", "vid"]
    assert not u_pad and c_pad.get("stage_pack_ctx_rows", 0) == 0          # a padded batch never meets the new entry points
    assert sum(c_pk.values()) <= sum(c_pad.values()) + 2
    assert c_pk.get("stage_pack_ctx_rows", 0) == 2 and c_pk.get("stage_rag_ctx_rows", 0) == 0      # a replacement, not an addition
    assert len(u_pk) == 2 and all(not a[0] and not a[2] for a in u_pk)     # mask-only calls: packed == dense == NULL


@pytest.mark.parametrize("fdt", [None, torch.float16])
def test_prefetcher_delivers_packed_streams(hip_device, fdt):
    from tvqaplus_amd.packed import PackedFeatures
    from tvqaplus_amd.prefetch import BatchPrefetcher
    from tvqaplus_amd.synth import make_batch
    host = [make_batch(packed=True, **dict(SHAPE, seed=40 + i, N=2 + i)) for i in range(3)]
    got = list(BatchPrefetcher(iter(host), hip_device, feature_dtype=fdt))
    torch.cuda.synchronize()
    assert len(got) == 3
    for h, d in zip(host, got):
        for key in ("sub_bert", "vid"):
            assert isinstance(d[key], PackedFeatures) and d[key].is_cuda and d[key].shape == h[key].shape
            assert d[key].lens is h[key].lens or np.array_equal(d[key].lens, h[key].lens)
            assert isinstance(d[key].lens, np.ndarray)                                            # the lengths stay on the host
            src = h[key].data if fdt is None else h[key].data.half()
            assert d[key].dtype == src.dtype and torch.equal(_bytes(d[key].data.cpu()), _bytes(src))
            assert float(d[key].data[d[key].P].abs().max()) == 0.0
        assert torch.equal(d.qas_bert.cpu(), h.qas_bert if fdt is None else h.qas_bert.half())
        assert "sub_mask" not in d and "vid_mask" not in d
