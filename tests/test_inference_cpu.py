"""CPU: the host side of the inference path -- kdpc_flow_propagate's argument checks (an
error code before any launch), the anchor sampling protocol and the ragged packing."""
import pytest
import torch

import kdpc_native

EINVAL = 1  # hipErrorInvalidValue
P = 0x1000  # a non-null pointer: every call below returns before anything reads it


def _fp(b=1, n=8, c=3, m_total=10, max_len=10, anchors=P, vals=P, qry=P, offsets=P, out=P,
        idx=None):
    lib = kdpc_native.load_library()
    return lib.kdpc_flow_propagate(b, n, c, m_total, max_len, anchors, vals, qry, offsets, out,
                                   idx, None)


def test_flow_propagate_rejects_invalid_sizes_without_launch():
    assert _fp(n=2) == EINVAL          # fewer than 3 anchors
    assert _fp(c=0) == EINVAL
    assert _fp(b=-1) == EINVAL
    assert _fp(b=65536) == EINVAL      # grid.y limit
    assert _fp(m_total=-1) == EINVAL
    assert _fp(max_len=-1) == EINVAL
    assert _fp(out=None) == EINVAL     # work to do and nowhere to write it
    for name in ("anchors", "vals", "qry", "offsets"):
        assert _fp(**{name: None}) == EINVAL, name


def test_flow_propagate_empty_work_is_a_noop():
    assert _fp(b=0, anchors=None, vals=None, qry=None, offsets=None, out=None) == 0
    assert _fp(m_total=0, max_len=0, anchors=None, vals=None, qry=None, offsets=None,
               out=None) == 0


def test_flow_propagate_binding_rejects_cpu_tensors():
    a = torch.zeros(1, 4, 3)
    with pytest.raises(kdpc_native.KdpcError):
        kdpc_native.flow_propagate(a, a, torch.zeros(5, 3), torch.tensor([0, 5]), 5)
    with pytest.raises(ValueError):  # offsets must hold B + 1 values
        kdpc_native.flow_propagate(a, a, torch.zeros(5, 3), torch.tensor([0, 2, 5]), 5)


def test_sample_anchors_protocol():
    from inference import sample_anchors
    g = torch.Generator().manual_seed(3)
    more, exact, fewer = sample_anchors([5000, 2048, 300], 2048, g)
    for idx, m in ((more, 5000), (exact, 2048), (fewer, 300)):
        assert idx.shape == (2048,) and idx.dtype == torch.int64
        assert int(idx.min()) >= 0 and int(idx.max()) < m
    # M >= N: a permutation prefix, so no row twice; M < N: with replacement
    assert more.unique().numel() == 2048
    assert exact.sort().values.tolist() == list(range(2048))
    assert fewer.unique().numel() <= 300
    with pytest.raises(ValueError):
        sample_anchors([10, 0], 4, g)


def test_sample_anchors_seed_reproduces_and_clouds_draw_independently():
    from inference import sample_anchors
    a = sample_anchors([4000, 4000, 100, 100], 512, torch.Generator().manual_seed(11))
    b = sample_anchors([4000, 4000, 100, 100], 512, torch.Generator().manual_seed(11))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # pc1 and pc2 of a pair (same length) are separate draws: real scans do not correspond
    assert not torch.equal(a[0], a[1])
    assert not torch.equal(a[2], a[3])
    c = sample_anchors([4000, 4000, 100, 100], 512, torch.Generator().manual_seed(12))
    assert not torch.equal(a[0], c[0])


def test_pack_scans_offsets_with_an_empty_cloud():
    from inference import pack_scans
    scans = [torch.arange(6.).reshape(2, 3), torch.zeros(0, 3), torch.arange(15.).reshape(5, 3)]
    packed, offsets, max_len = pack_scans(scans)
    assert offsets.dtype == torch.int64 and offsets.tolist() == [0, 2, 2, 7]
    assert max_len == 5 and packed.shape == (7, 3) and packed.is_contiguous()
    for i, s in enumerate(scans):
        assert torch.equal(packed[offsets[i]:offsets[i + 1]], s)
    packed, offsets, max_len = pack_scans([torch.zeros(0, 3)])
    assert offsets.tolist() == [0, 0] and max_len == 0 and packed.shape == (0, 3)
    with pytest.raises(ValueError):
        pack_scans([torch.zeros(4, 2)])
