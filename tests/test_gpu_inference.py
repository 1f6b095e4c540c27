"""GPU: the inference path -- kdpc_flow_propagate (the ragged, fused 3-NN + inverse-distance
blend) against the pinned kernels it fuses, FlowPredictor's graph replay against the eager
eval forward, predict_dense against the hand-written composition and evaluate_dense against
metrics computed by hand, on real KITTI points (tests/golden/data_path_ref.npz)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"


@pytest.fixture(scope="module")
def nat():
    import kdpc_native
    kdpc_native.load_library()
    return kdpc_native


@pytest.fixture(scope="module")
def model():
    from models_bid_pointconv import PointConvBidirection
    torch.manual_seed(0)
    return PointConvBidirection().to(DEV).eval()


@pytest.fixture(scope="module")
def scenes():
    g = np.load(os.path.join(GOLDEN, "data_path_ref.npz"))
    return {k: (torch.from_numpy(g[f"{k}_noground_pc1"]).to(DEV),
                torch.from_numpy(g[f"{k}_noground_pc2"]).to(DEV)) for k in ("k1", "k3")}


def _problem(n, lens, c, seed):
    """Lidar-like coordinates (tens of metres from the origin).  Every anchor appears twice
    (rows j and j + ceil(n/2): the lower index must win each tie) and every third query sits
    exactly on an anchor (distance 0: the 1e-10 clamp)."""
    g = torch.Generator().manual_seed(seed)
    b = len(lens)
    half = (n + 1) // 2
    base = torch.randn(b, half, 3, generator=g) * torch.tensor([20., 2., 30.]) + \
        torch.tensor([5., 0., 40.])
    anchors = torch.cat([base, base], 1)[:, :n].contiguous()
    vals = torch.randn(b, n, c, generator=g)
    qs = []
    for i, m in enumerate(lens):
        q = torch.randn(m, 3, generator=g) * torch.tensor([20., 2., 30.]) + \
            torch.tensor([5., 0., 40.])
        on = torch.arange(0, m, 3)
        q[on] = anchors[i, torch.randint(n, (on.numel(),), generator=g)]
        qs.append(q)
    off = [0]
    for m in lens:
        off.append(off[-1] + m)
    return (anchors.to(DEV), vals.to(DEV), [q.to(DEV) for q in qs],
            torch.tensor(off, dtype=torch.int64).to(DEV))


# N: the minimum, an odd size, one past a 1024-anchor tile, two tiles; lengths: an empty cloud,
# a single row, a cloud straddling a 256-row block; C: the scalar (3, 6) and 16-byte (4) value
# paths; max_len equal to and larger than the longest cloud
@pytest.mark.parametrize("c", [3, 4, 6])
@pytest.mark.parametrize("lens", [[0, 1, 257], [300, 0, 255]])
@pytest.mark.parametrize("n", [3, 5, 1025, 2048])
def test_flow_propagate_is_three_nn_plus_idw_blend(nat, n, lens, c):
    anchors, vals, qs, offsets = _problem(n, lens, c, seed=n + c)
    qry = torch.cat(qs, 0).contiguous()
    out, idx = nat.flow_propagate(anchors, vals, qry, offsets, max(lens), return_idx=True)
    assert out.shape == (sum(lens), c) and idx.shape == (sum(lens), 3)
    assert idx.dtype == torch.int32
    # a looser bound on the lengths (more blocks, all past the clouds' ends) and no idx_out
    for max_len in (max(lens), max(lens) + 1000):
        assert torch.equal(nat.flow_propagate(anchors, vals, qry, offsets, max_len), out)
    out2, idx2 = nat.flow_propagate(anchors, vals, qry, offsets, max(lens) + 1000,
                                    return_idx=True)
    assert torch.equal(out2, out) and torch.equal(idx2, idx)
    off = offsets.tolist()
    ties = 0
    for i, q in enumerate(qs):
        if q.shape[0] == 0:
            continue
        a, v = anchors[i:i + 1], vals[i:i + 1]
        ref_idx = nat.three_nn(q[None], a)[1]
        ref_out = nat.idw_blend_fwd(a, q[None], v, ref_idx)[0]
        assert torch.equal(idx[off[i]:off[i + 1]], ref_idx[0])
        assert torch.equal(out[off[i]:off[i + 1]], ref_out[0])
        ties += int((ref_idx[0, :, 0] < (n + 1) // 2).sum())
    # every anchor of the upper half has an identical twin below it: the nearest is never one
    assert ties == sum(lens)
    # independent arithmetic: the same formula in float64 on the returned indices; 1e-5 is
    # the project's layer tolerance (the f32 chain alone sits near 1e-7 max|vals|)
    A, V, Q = (t.double().cpu().numpy() for t in (anchors, vals, qry))
    I = idx.cpu().numpy().astype(np.int64)
    cloud = np.repeat(np.arange(len(lens)), lens)
    assert I.min(initial=0) >= 0 and I.max(initial=0) < n
    d = np.maximum(np.linalg.norm(A[cloud[:, None], I] - Q[:, None], axis=-1), 1e-10)
    w = (1.0 / d) / (1.0 / d).sum(-1, keepdims=True)
    want = (w[..., None] * V[cloud[:, None], I]).sum(1)
    err = np.abs(out.cpu().numpy() - want).max(initial=0.0)
    assert err <= 1e-5 * np.abs(V).max(), err


def test_flow_propagate_nan_query_reads_anchor_zero(nat):
    anchors, vals, qs, offsets = _problem(40, [5], 3, seed=1)
    q = qs[0].clone()
    q[2] = float("nan")
    _, idx = nat.flow_propagate(anchors, vals, q, offsets, 5, return_idx=True)
    assert torch.equal(idx, nat.three_nn(q[None], anchors)[1][0])
    assert idx[2].tolist() == [0, 0, 0]


def _eager(model, p1, p2):
    with torch.no_grad():
        return model(p1, p2, p1, p2)[0][0].permute(0, 2, 1).contiguous()


def _pair(scene, n, seed):
    g = torch.Generator().manual_seed(seed)
    p1, p2 = scene
    i1 = torch.randperm(p1.shape[0], generator=g)[:n].to(DEV)
    i2 = torch.randperm(p2.shape[0], generator=g)[:n].to(DEV)
    return p1[i1][None].contiguous(), p2[i2][None].contiguous()


@pytest.fixture(scope="module")
def batches(model, scenes):
    """Two different (pc1, pc2) batches at B=1, N=2048 and their eager eval flows."""
    bs = [_pair(scenes["k1"], 2048, 1), _pair(scenes["k3"], 2048, 2)]
    return bs, [_eager(model, *b) for b in bs]


def test_predictor_graph_replay_equals_eager_forward(model, batches):
    from inference import FlowPredictor
    bs, want = batches
    pred = FlowPredictor(model, 1, 2048, graph=True)
    assert pred.graph is not None
    for _ in range(2):  # both batches through the one captured graph, twice
        for b, w in zip(bs, want):
            got = pred.predict(*b)
            assert got.shape == (1, 2048, 3) and torch.equal(got, w)
    eager = FlowPredictor(model, 1, 2048, graph=False)
    assert eager.graph is None and torch.equal(eager.predict(*bs[0]), want[0])
    with pytest.raises(ValueError):
        pred.predict(bs[0][0][:, :1024], bs[0][1][:, :1024])


def test_predictor_prefetch_hit_and_miss_equal_eager(model, batches):
    from inference import FlowPredictor
    bs, want = batches
    for graph in (True, False):
        pred = FlowPredictor(model, 1, 2048, graph=graph, prefetch=True)
        # call 1 announces batch 1; call 2 is fed what was prefetched for it; call 3's batch
        # was not announced (call 2 announced nothing): the plan is recomputed
        assert torch.equal(pred.predict(*bs[0], next_batch=bs[1]), want[0])
        assert pred._hit(bs[1])
        assert torch.equal(pred.predict(*bs[1]), want[1])
        assert not pred._hit(bs[0])
        assert torch.equal(pred.predict(*bs[0]), want[0])


def _compose_dense(nat, model, s1, s2, n, seed):
    """predict_dense written out by hand from the pinned pieces."""
    from inference import sample_anchors
    i1, i2 = sample_anchors([s1.shape[0], s2.shape[0]], n, torch.Generator().manual_seed(seed))
    a1, a2 = s1[i1.to(DEV)][None].contiguous(), s2[i2.to(DEV)][None].contiguous()
    aflow = _eager(model, a1, a2)
    idx = nat.three_nn(s1[None], a1)[1]
    return nat.idw_blend_fwd(a1, s1[None].contiguous(), aflow, idx)[0][0], i1, i2, aflow


@pytest.mark.parametrize("key,m", [("k1", 2710), ("k3", 2296)])
def test_predict_dense_equals_hand_written_composition(nat, model, scenes, key, m):
    """k1: more points than anchors (sampled without replacement); k3: fewer (with)."""
    from inference import FlowPredictor
    s1, s2 = scenes[key]
    assert s1.shape == (m, 3)
    pred = FlowPredictor(model, 1, 2048, graph=True)
    want, i1, i2, aflow = _compose_dense(nat, model, s1, s2, 2048, seed=5)
    assert (i1.unique().numel() == 2048) == (m >= 2048)
    for _ in range(2):  # the same seed gives the same result
        flow, offsets, (g1, g2), gflow = pred.predict_dense(
            [s1], [s2], torch.Generator().manual_seed(5))
        assert flow.shape == (m, 3) and offsets.tolist() == [0, m]
        assert offsets.dtype == torch.int64 and offsets.is_cuda
        assert torch.equal(g1.cpu(), i1[None]) and torch.equal(g2.cpu(), i2[None])
        assert torch.equal(gflow, aflow)
        assert torch.equal(flow, want)


@pytest.fixture(scope="module")
def kitti(tmp_path_factory):
    g = np.load(os.path.join(GOLDEN, "data_path_ref.npz"))
    root = tmp_path_factory.mktemp("kitti")
    for s in (1, 2, 3):
        d = root / "kitti_processed" / ("%06d" % s)
        d.mkdir(parents=True)
        np.save(d / "pc1.npy", g[f"k{s}_pc1"])
        np.save(d / "pc2.npy", g[f"k{s}_pc2"])
    with open(root / "KITTI_mapping.txt", "w") as fd:
        fd.write("".join(("x\n" if v else "\n") for v in g["mapping_nonempty"]))
    calib = root / "calib"
    calib.mkdir()
    for s in (1, 2, 3):
        (calib / ("%06d.txt" % s)).write_text(str(g[f"calib{s}_p_rect_02"]) + "\n")
    return root


def test_evaluate_dense_equals_metrics_by_hand(model, kitti):
    import datasets as D
    import transforms as T
    from evaluate_bid_pointconv import evaluate_dense
    from evaluation_utils import evaluate_2d, evaluate_3d
    from inference import FlowPredictor
    from utils import geometry
    ds = D.KITTI(train=False, num_points=0, data_root=str(kitti),
                 transform=T.ProcessData(dict(DEPTH_THRESHOLD=35., NO_CORR=True), 0, False))
    calib = str(kitti / "calib")
    got = evaluate_dense(model, D.DeviceLoader(ds, 1, "cuda"), 2048, seed=9, calib_dir=calib)
    pred = FlowPredictor(model, 1, 2048, graph=False)
    gen = torch.Generator().manual_seed(9)
    rows, points = [], 0
    for pos1, pos2, _, _, flow, paths in D.DeviceLoader(ds, 1, "cpu"):
        dense = pred.predict_dense([pos1[0].to(DEV)], [pos2[0].to(DEV)], gen)[0]
        assert dense.shape == pos1[0].shape
        pc1, sf, full = pos1.numpy(), flow.numpy(), dense[None].cpu().numpy()
        fp, fg = geometry.get_batch_2d_flow(pc1, pc1 + sf, pc1 + full, paths, calib_dir=calib)
        rows.append([*evaluate_3d(full, sf), *evaluate_2d(fp, fg)])
        points += pos1.shape[1]
    want = np.mean(np.array(rows, dtype=np.float64), 0)
    keys = ("EPE3D", "ACC3DS", "ACC3DR", "Outliers3D", "EPE2D", "ACC2D")
    np.testing.assert_allclose([got[k] for k in keys], want, rtol=1e-5, atol=1e-7)
    assert got["batches"] == got["samples"] == len(rows) == 2 and got["points"] == points
