"""CPU-side checks of packed context features (tvqaplus_amd/packed.py, csrc/packed.hip, include/stage_hip.h): the format against its own
host specification (``unpad_host``), the collate, the host restatement of the packed source-row table, the shard functions, and the two
C entry points' argument checks -- none of which needs a GPU."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

SYMBOLS = ["stage_pack_ctx_rows", "stage_pack_unpack"]
ERR_SHAPE = -1          # include/stage_hip.h: STAGE_ERR_SHAPE


def _padded(N=3, Li=4, L=5, K=8, seed=0, dtype=torch.float32):
    """A padded (N, Li, L, K) tensor whose lens hold 0, L, 1 and a hole (an all-zero row) inside a prefix."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(0, L + 1, (N, Li), generator=g).numpy().astype(np.int32)
    lens[0, 0], lens[0, 1], lens[0, 2], lens[1, 0] = 0, L, 1, 4
    x = torch.randn(N, Li, L, K, generator=g)
    x = x * (torch.arange(L).view(1, 1, L) < torch.from_numpy(lens.astype(np.int64)).unsqueeze(-1)).unsqueeze(-1)
    x[1, 0, 1] = 0.0                                                  # the hole: position 1 of a frame of length 4
    return x.to(dtype), lens


def test_from_padded_round_trips_and_reproduces_the_prefix_mask():
    from tvqaplus_amd.packed import PackedFeatures
    x, lens = _padded()
    pf = PackedFeatures.from_padded(x, lens, check=True)
    assert set([0, 5, 1]) <= set(lens.reshape(-1).tolist())
    assert pf.shape == (3, 4, 5, 8) and pf.dtype == torch.float32 and pf.device.type == "cpu" and not pf.is_cuda
    assert pf.data.shape == (int(lens.sum()) + 1, 8) and pf.data.is_contiguous()
    assert float(pf.data[pf.P].abs().max()) == 0.0                    # the zero row
    dense, mask = pf.unpad_host()
    assert torch.equal(dense, x)
    want = (torch.arange(5).view(1, 1, 5) < torch.from_numpy(lens.astype(np.int64)).unsqueeze(-1)).float()
    assert mask.dtype == torch.float32 and torch.equal(mask, want)
    st = int(pf.starts()[1 * 4 + 0])
    assert float(pf.data[st + 1].abs().max()) == 0.0 and float(pf.data[st + 2].abs().max()) > 0      # the hole stays a row
    bad = x.clone()
    bad[0, 2, 3, 0] = 1.0                                             # behind len = 1
    with pytest.raises(AssertionError):
        PackedFeatures.from_padded(bad, lens, check=True)
    h = pf.to(torch.float16)
    assert h.dtype == torch.float16 and torch.equal(h.data, pf.data.half()) and float(h.data[h.P].abs().max()) == 0.0
    assert np.array_equal(h.lens, pf.lens) and h.lens.dtype == np.int32


def test_from_sequences_equals_from_padded_of_the_padded_lists():
    from tvqaplus_amd.packed import PackedFeatures
    g = torch.Generator().manual_seed(1)
    L, K = 6, 4
    counts = [[3, 0, 6, 1], [2, 2], [6, 0, 0, 5]]
    seqs = [[torch.randn(c, K, generator=g) for c in ex] for ex in counts]
    # the reference's pad_sequences_2d, restated: zero-fill, copy every frame's rows, lengths on the side
    N, Li = len(seqs), max(len(ex) for ex in seqs)
    x, lens = torch.zeros(N, Li, L, K), np.zeros((N, Li), dtype=np.int32)
    for n, ex in enumerate(seqs):
        for i, t in enumerate(ex):
            x[n, i, :len(t)], lens[n, i] = t, len(t)
    a = PackedFeatures.from_sequences(seqs, L)
    b = PackedFeatures.from_padded(x, lens, check=True)
    assert a.shape == b.shape and np.array_equal(a.lens, b.lens) and torch.equal(a.data, b.data)
    out = torch.full((a.P + 9, K), float("nan"))
    c = PackedFeatures.from_sequences(seqs, L, Li=5, out=out)
    assert c.data.data_ptr() == out.data_ptr() and torch.equal(c.data, a.data) and c.shape == (3, 5, 6, 4)
    assert torch.isnan(out[a.P + 1:]).all()                           # nothing behind the zero row is touched
    with pytest.raises(ValueError):
        PackedFeatures.from_sequences(seqs, 5)                        # a frame of 6 rows in rows of 5


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_nbytes_is_the_rows_plus_the_zero_row(dtype):
    from tvqaplus_amd.packed import PackedFeatures
    x, lens = _padded(dtype=dtype)
    pf = PackedFeatures.from_padded(x, lens)
    assert pf.nbytes == (int(lens.sum()) + 1) * 8 * torch.empty(0, dtype=dtype).element_size()
    assert pf.nbytes == pf.data.numel() * pf.data.element_size()


def test_lens_outside_the_row_length_raise():
    from tvqaplus_amd.packed import PackedFeatures
    x, lens = _padded()
    for v in (-1, 6):
        bad = lens.copy()
        bad[2, 3] = v
        with pytest.raises(ValueError):
            PackedFeatures.from_padded(x, bad)
        with pytest.raises(ValueError):
            PackedFeatures(torch.zeros(max(int(bad.sum()), 0) + 1, 8), bad, 5)
    with pytest.raises(ValueError):
        PackedFeatures(torch.zeros(int(lens.sum()) + 2, 8), lens, 5)   # a row too many


@pytest.mark.parametrize("halo", [6, 1 << 20])
def test_packed_source_rows_gather_what_the_padded_source_rows_gather(halo):
    from tvqaplus_amd import ragged
    from tvqaplus_amd.packed import PackedFeatures
    x, lens = _padded(N=3, Li=4, L=9, K=8, seed=4)
    lens[0, 1] = 9
    lens[2, 0] = 5                                                    # len + halo > L
    x, _ = PackedFeatures.from_padded(x, lens).unpad_host()          # zeros behind the edited lens
    pf = PackedFeatures.from_padded(x, lens, check=True)
    ct = ragged.CtxTables(lens, 9, halo)
    src_p, src_d = ct.src_rows_packed_host(pf.ptab(), pf.P), ct.src_rows_host()
    assert src_p.dtype == np.int32 and src_p.shape == src_d.shape == (ct.U,) and ct.U > 0
    assert int(src_p.min()) >= 0 and int(src_p.max()) <= pf.P and (src_p == pf.P).any()
    assert torch.equal(pf.data[torch.from_numpy(src_p).long()], x.view(-1, 8)[torch.from_numpy(src_d).long()])


def test_slices_and_shards_unpad_to_the_shard_of_the_unpadded_batch():
    from tvqaplus_amd import parallel
    from tvqaplus_amd.packed import PackedFeatures
    from tvqaplus_amd.synth import make_batch
    kw = dict(N=5, Li=6, Lr=8, Lw=10, Lqa=12, wd_size=16, vfeat_size=12, seed=7, empty_frames=True)
    pad, pk = make_batch(**kw), make_batch(packed=True, **kw)
    assert isinstance(pk.sub_bert, PackedFeatures) and isinstance(pk.vid, PackedFeatures)
    assert "sub_mask" not in pk and "vid_mask" not in pk and torch.equal(pk.qas_bert, pad.qas_bert)
    for key, mkey in (("sub_bert", "sub_mask"), ("vid", "vid_mask")):
        d, m = pk[key].unpad_host()
        assert torch.equal(d, pad[key]) and torch.equal(m, pad[mkey])
        for lo, hi in ((0, 5), (1, 3), (4, 5), (2, 2)):
            s = pk[key].slice_examples(lo, hi)
            ds, ms = s.unpad_host()
            assert torch.equal(ds, pad[key][lo:hi]) and torch.equal(ms, pad[mkey][lo:hi])
            assert s.data.shape[0] == int(pk[key].lens[lo:hi].sum()) + 1 and float(s.data[s.P].abs().max()) == 0.0
    for rank in range(3):
        a, b = parallel.shard_batch(pk, rank, 3), parallel.shard_batch(pad, rank, 3)
        for key, mkey in (("sub_bert", "sub_mask"), ("vid", "vid_mask")):
            d, m = a[key].unpad_host()
            assert torch.equal(d, b[key]) and torch.equal(m, b[mkey])
            assert np.array_equal(a.mask_host[mkey[:3] + "_len"], a[key].lens)
        assert torch.equal(a.qas_bert, b.qas_bert) and a.qid == b.qid
    for rank in (0, 3, 9):                                            # 5 example blocks x 2 candidate parts
        lay = parallel.CandidateLayout(5, rank, 10)
        a, b = lay.shard(pk), lay.shard(pad)
        for key, mkey in (("sub_bert", "sub_mask"), ("vid", "vid_mask")):
            d, m = a[key].unpad_host()
            assert torch.equal(d, b[key]) and torch.equal(m, b[mkey])
        assert torch.equal(a.qas_bert, b.qas_bert) and a.cand_offset == b.cand_offset


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from tvqaplus_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", ROOT, "-j8"], stdout=subprocess.DEVNULL)
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    from tvqaplus_amd import _lib
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    hdr = open(os.path.join(ROOT, "include", "stage_hip.h")).read()
    assert all(("int %s(" % name) in hdr for name in SYMBOLS)
    assert lib.stage_hip_abi_version() == 7


def test_bad_shapes_are_refused_before_any_launch(lib):
    """No GPU here: a call that got as far as a launch would not return STAGE_ERR_SHAPE."""
    buf = torch.zeros(4096, dtype=torch.uint8)       # never read: every call below returns before a launch
    p = buf.data_ptr()
    p += (-p) % 16
    for rb in (12, 4, 4104):
        assert lib.stage_pack_unpack(p, p, p, None, 7, 5, rb, None) == ERR_SHAPE, rb
        assert lib.stage_pack_unpack(p, p, p, p, 7, 5, rb, None) == ERR_SHAPE, rb
    assert lib.stage_pack_unpack(p, p, p, None, 7, 0, 16, None) == ERR_SHAPE
    assert lib.stage_pack_unpack(None, p, None, p, 7, 0, 0, None) == ERR_SHAPE
    assert lib.stage_pack_unpack(p, p, p, None, 1 << 16, 1 << 15, 16, None) == ERR_SHAPE       # frames * L = 2^31
    assert lib.stage_pack_unpack(None, p, None, p, 1 << 16, 1 << 15, 0, None) == ERR_SHAPE
    assert lib.stage_pack_unpack(p + 4, p, p, None, 7, 5, 16, None) == ERR_SHAPE               # a base that is not 8-byte aligned
    assert lib.stage_pack_unpack(p, p, p + 4, None, 7, 5, 16, None) == ERR_SHAPE
    assert lib.stage_pack_ctx_rows(p, p, 7, 0, 3, p, None) == ERR_SHAPE
    assert lib.stage_pack_ctx_rows(p, p, 1 << 16, 1 << 15, 3, p, None) == ERR_SHAPE
    assert lib.stage_pack_ctx_rows(p, p, 0, 5, 3, p, None) == 0                                # no frames: nothing to do
    assert lib.stage_pack_unpack(p, p, p, None, 0, 5, 16, None) == 0
