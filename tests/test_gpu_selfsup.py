"""The self-supervised loss on the GPU: the fused Chamfer kernels (csrc/chamfer.hip) against
three_nn and float64, the loss (selfsup.py) against a float64 restatement, and the graphed
self-supervised step against the eager one."""
import copy
import math
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

SCALE = torch.tensor([20., 2., 30.])
SHIFT = torch.tensor([5., 0., 40.])
# the minimum three_nn takes, odd sizes on both sides of a 256-row block, one past the kernel's
# 1024-point LDS tile on either side, two tiles against a partial one
SIZES = [(3, 3), (5, 257), (257, 5), (1025, 1024), (1024, 1025), (2048, 300)]


def _lidar(g, *shape):
    """Lidar-like coordinates: tens of metres from the origin."""
    return torch.randn(*shape, 3, generator=g) * SCALE + SHIFT


def _clouds(bsz, n, m, seed):
    """As test_gpu_inference._problem: every point of b is present twice (rows j and
    j + ceil(m/2): the lower index must win) and every third row of a lies exactly on a point
    of b (distance 0)."""
    g = torch.Generator().manual_seed(seed)
    half = (m + 1) // 2
    base = _lidar(g, bsz, half)
    b = torch.cat([base, base], 1)[:, :m].contiguous()
    a = _lidar(g, bsz, n)
    on = torch.arange(0, n, 3)
    for i in range(bsz):
        a[i, on] = b[i, torch.randint(m, (on.numel(),), generator=g)]
    return a.to(DEV), b.to(DEV)


def _rows(x, idx):
    """x (B,M,3), idx (B,N) -> x[b, idx[b,n]] (B,N,3)."""
    return torch.gather(x, 1, idx.long()[..., None].expand(-1, -1, 3))


# ------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("bsz", [1, 3])
@pytest.mark.parametrize("n,m", SIZES)
def test_forward_is_three_nn_first_column(n, m, bsz):
    import kdpc_native as nat
    a, b = _clouds(bsz, n, m, seed=n + m + bsz)
    dist_ab, idx_ab, dist_ba, idx_ba = nat.chamfer_fwd(a, b)
    assert dist_ab.shape == (bsz, n) and idx_ab.shape == (bsz, n)
    assert dist_ba.shape == (bsz, m) and idx_ba.shape == (bsz, m)
    assert idx_ab.dtype == torch.int32 and idx_ba.dtype == torch.int32
    d3, i3 = nat.three_nn(a, b)
    assert torch.equal(dist_ab, d3[..., 0].contiguous())
    assert torch.equal(idx_ab, i3[..., 0].contiguous())
    d3, i3 = nat.three_nn(b, a)
    assert torch.equal(dist_ba, d3[..., 0].contiguous())
    assert torch.equal(idx_ba, i3[..., 0].contiguous())
    # ties occurred and the lower index won each: the rows of a placed on a point of b are at
    # distance 0 from it and from its copy half a cloud later
    half = (m + 1) // 2
    on = torch.arange(0, n, 3, device=DEV)
    assert (dist_ab[:, on] == 0).all()
    twin = idx_ab.long() + half
    has_twin = twin < m
    assert has_twin[:, on].any()
    same = (_rows(b, twin.clamp(max=m - 1)) == _rows(b, idx_ab)).all(-1)
    assert same[has_twin].all()
    assert (idx_ab < half).all()


@pytest.mark.parametrize("bsz", [1, 3])
@pytest.mark.parametrize("n,m", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_forward_tiny_clouds_against_float64(n, m, bsz):
    """Sizes three_nn cannot serve.  Small-integer coordinates: every distance is exact in
    f32, so the float64 brute force (lowest index on ties) must be met exactly."""
    import kdpc_native as nat
    g = torch.Generator().manual_seed(10 * n + m + bsz)
    a = torch.randint(-4, 5, (bsz, n, 3), generator=g).float()
    b = torch.randint(-4, 5, (bsz, m, 3), generator=g).float()
    if m == 2:
        b[0, 1] = b[0, 0]  # a tie for every row of a
    got = nat.chamfer_fwd(a.to(DEV), b.to(DEV))

    def brute(q, r):
        d = ((q.double()[:, :, None] - r.double()[:, None]) ** 2).sum(-1)
        dmin = d.min(-1).values
        cand = torch.where(d == dmin[..., None], torch.arange(r.shape[1]), r.shape[1])
        return dmin, cand.min(-1).values
    for (dist, idx), (rd, ri) in zip((got[:2], got[2:]), (brute(a, b), brute(b, a))):
        assert torch.equal(dist.cpu().double(), rd)
        assert torch.equal(idx.cpu().long(), ri)


def test_forward_nan_row():
    """A NaN distance never wins: the row gets index 0, is nobody's neighbour, and every
    other row of a is as without it."""
    import kdpc_native as nat
    a, b = _clouds(2, 300, 257, seed=7)
    ref = nat.chamfer_fwd(a, b)
    a2 = a.clone()
    a2[1, 17, 1] = float("nan")
    dist_ab, idx_ab, dist_ba, idx_ba = nat.chamfer_fwd(a2, b)
    assert idx_ab[1, 17] == 0 and dist_ab[1, 17] == math.inf
    keep = torch.ones(2, 300, dtype=torch.bool, device=DEV)
    keep[1, 17] = False
    assert torch.equal(dist_ab[keep], ref[0][keep]) and torch.equal(idx_ab[keep], ref[1][keep])
    assert (idx_ab >= 0).all() and (idx_ab < 257).all()
    assert (idx_ba >= 0).all() and (idx_ba < 300).all()
    assert (idx_ba[1] != 17).all()
    assert torch.equal(dist_ba[0], ref[2][0]) and torch.equal(idx_ba[0], ref[3][0])
    assert not torch.isnan(dist_ba).any()


# ----------------------------------------------------------------------------- backward
def _grad_reference(x, y, idx_xy, g_xy, idx_yx, g_yx):
    """float64, for the gradient with respect to x of sum g_xy ||x - y[idx_xy]||^2 +
    sum g_yx ||y - x[idx_yx]||^2 with the indices held fixed: (autograd gradient, number of
    terms k of every row, S = sum |term| per element)."""
    x64 = x.double().requires_grad_()
    y64 = y.double()
    loss = (g_xy.double() * ((x64 - _rows(y64, idx_xy)) ** 2).sum(-1)).sum() + \
        (g_yx.double() * ((y64 - _rows(x64, idx_yx)) ** 2).sum(-1)).sum()
    (grad,) = torch.autograd.grad(loss, x64)
    xd = x.double()
    direct = 2 * g_xy.double()[..., None] * (xd - _rows(y64, idx_xy))
    routed = 2 * g_yx.double()[..., None] * (_rows(xd, idx_yx) - y64)
    where = idx_yx.long()[..., None].expand(-1, -1, 3)
    s = direct.abs().scatter_add(1, where, routed.abs())
    k = torch.ones_like(direct).scatter_add(1, where, torch.ones_like(routed))
    return grad, k, s


def _upstream(g, bsz, n):
    """Random upstream gradients (B,n) of both signs with exact zeros among them (a lone
    value is negative)."""
    x = torch.randn(bsz, n, generator=g)
    x[:, 1::5] = 0
    x[:, 0] = -(x[:, 0].abs() + 0.5)
    return x


@pytest.mark.parametrize("bsz", [1, 3])
@pytest.mark.parametrize("n,m", SIZES + [(2048, 1), (1, 2048)])
def test_backward_against_float64(n, m, bsz):
    """|got - ref| <= (k + 4) 2^-23 S per element, k = the row's number of terms, S = sum |term|
    in float64: sequential f32 summation of k once-rounded terms stays within (k + 2) 2^-24 S;
    the bound is twice that.  (2048, 1) / (1, 2048): one point receives every row, a CSR run
    of 2048 next to rows with none."""
    import kdpc_native as nat
    g = torch.Generator().manual_seed(100 + n + m + bsz)
    if min(n, m) >= 3:
        a, b = _clouds(bsz, n, m, seed=n + m + bsz)
    else:
        a, b = _lidar(g, bsz, n).to(DEV), _lidar(g, bsz, m).to(DEV)
    _, idx_ab, _, idx_ba = nat.chamfer_fwd(a, b)
    g_ab, g_ba = _upstream(g, bsz, n).to(DEV), _upstream(g, bsz, m).to(DEV)
    csr_ba, csr_ab = nat.csr_of(idx_ba, n), nat.csr_of(idx_ab, m)
    da = nat.chamfer_bwd(a, b, idx_ab, g_ab, csr_ba, g_ba)
    db = nat.chamfer_bwd(b, a, idx_ba, g_ba, csr_ab, g_ab)
    assert da.shape == (bsz, n, 3) and db.shape == (bsz, m, 3)
    for got, ref in ((da, _grad_reference(a, b, idx_ab, g_ab, idx_ba, g_ba)),
                     (db, _grad_reference(b, a, idx_ba, g_ba, idx_ab, g_ab))):
        grad, k, s = ref
        err = (got.double() - grad).abs()
        bound = (k + 4) * 2.0 ** -23 * s
        worst = (err / bound.clamp(min=1e-300)).max().item()
        print(f"n={n} m={m} B={bsz}: max err/bound {worst:.3f}, max k {int(k.max())}")
        assert (err <= bound).all(), worst
    # one direction alone (NULL g_ba / CSR) is the two-directional form with g_ba = 0
    zero_ba, zero_ab = torch.zeros_like(g_ba), torch.zeros_like(g_ab)
    assert torch.equal(nat.chamfer_bwd(a, b, idx_ab, g_ab),
                       nat.chamfer_bwd(a, b, idx_ab, g_ab, csr_ba, zero_ba))
    assert torch.equal(nat.chamfer_bwd(b, a, idx_ba, g_ba),
                       nat.chamfer_bwd(b, a, idx_ba, g_ba, csr_ab, zero_ab))
    # deterministic
    assert torch.equal(nat.chamfer_bwd(a, b, idx_ab, g_ab, csr_ba, g_ba), da)
    assert torch.equal(nat.chamfer_bwd(b, a, idx_ba, g_ba, csr_ab, g_ab), db)


def test_exact_zeros():
    """pc2 = the first cloud moved by t (in f32) and shuffled, flow = t: the warped cloud is
    pc2 bit for bit, so both Chamfer distances and the flow's gradient are exactly 0 tens of
    metres from the origin; a constant flow has smoothness 0 with gradient 0."""
    import selfsup
    g = torch.Generator().manual_seed(5)
    bsz, n = 2, 1000
    pc1 = _lidar(g, bsz, n).to(DEV)
    t = torch.tensor([0.53, -0.21, 1.37], device=DEV)
    perm = torch.randperm(n, generator=g).to(DEV)
    pc2 = (pc1 + t)[:, perm].contiguous()
    flow = t.expand(bsz, n, 3).clone().requires_grad_()
    dist_ab, dist_ba = selfsup.chamfer_distance(pc1 + flow, pc2)
    assert (dist_ab == 0).all() and (dist_ba == 0).all()
    (dist_ab.sum() + 3 * dist_ba.sum()).backward()
    assert (flow.grad == 0).all()
    flow.grad = None
    smooth = selfsup.flow_smoothness(pc1, flow)
    assert smooth.item() == 0
    smooth.backward()
    assert (flow.grad == 0).all()
    flow.grad = None
    cn = lambda x: x.permute(0, 2, 1)  # noqa: E731
    loss = selfsup.multiScaleChamferSmooth([cn(flow)], [cn(pc1)], [cn(pc2)])
    assert loss.shape == (1,) and loss.item() == 0
    loss.backward()
    assert (flow.grad == 0).all()


# --------------------------------------------------------------------------------- loss
def _loss_reference(flows, pc1, pc2, alpha, f_chamfer, f_smooth, k):
    """selfsup.multiScaleChamferSmooth in float64, the Chamfer and kNN indices taken from the
    HIP ops on the f32 inputs (the discrete choices are replayed)."""
    import selfsup
    from pointconv_util import knn_point
    total = 0
    for i, fl in enumerate(flows):
        p1 = pc1[i].permute(0, 2, 1).contiguous()
        p2 = pc2[i].permute(0, 2, 1).contiguous()
        with torch.no_grad():
            _, _, idx_ab, idx_ba = selfsup.chamfer_neighbours(
                p1 + fl.detach().float().permute(0, 2, 1), p2)
            knn = knn_point(k, p1, p1).long()
        f = fl.permute(0, 2, 1)
        warp = p1.double() + f
        chamfer = ((warp - _rows(p2.double(), idx_ab)) ** 2).sum(-1).sum(1).mean() + \
            ((p2.double() - _rows(warp, idx_ba)) ** 2).sum(-1).sum(1).mean()
        bsz, n, _ = f.shape
        nb = _rows(f, knn.reshape(bsz, n * k)).reshape(bsz, n, k, 3)
        smooth = (torch.norm(nb - f[:, :, None], dim=3).sum(2) / (k - 1)).sum(1).mean()
        total = total + alpha[i] * (f_chamfer * chamfer + f_smooth * smooth)
    return total


def test_loss_against_float64():
    import selfsup
    g = torch.Generator().manual_seed(11)
    bsz, sizes = 2, (512, 256, 128, 64)
    cn = lambda x: x.permute(0, 2, 1)  # noqa: E731
    pc1 = [cn(_lidar(g, bsz, n).to(DEV)) for n in sizes]
    pc2 = [cn(_lidar(g, bsz, n).to(DEV)) for n in sizes]
    flows = [torch.randn(bsz, 3, n, generator=g).to(DEV).requires_grad_() for n in sizes]
    alpha, f_chamfer, f_smooth, k = [0.02, 0.04, 0.08, 0.16], 1.0, 0.7, 9
    loss = selfsup.multiScaleChamferSmooth(flows, pc1, pc2, alpha, f_chamfer, f_smooth, k)
    grads = torch.autograd.grad(loss.sum(), flows)
    flows64 = [f.detach().double().requires_grad_() for f in flows]
    ref = _loss_reference(flows64, pc1, pc2, alpha, f_chamfer, f_smooth, k)
    grads64 = torch.autograd.grad(ref, flows64)
    rel = abs(loss.item() - ref.item()) / abs(ref.item())
    print(f"loss {loss.item():.9g} ref {ref.item():.12g} rel {rel:.3g}")
    assert math.isfinite(loss.item()) and rel < 1e-5
    for n, got, want in zip(sizes, grads, grads64):
        err = (got.double() - want).abs().max().item() / want.abs().max().item()
        print(f"level N={n}: grad err / max |grad| {err:.3g}")
        assert err < 1e-5
    # the default weights (f_smooth = 1) are the same sum
    d = selfsup.multiScaleChamferSmooth(flows, pc1, pc2)
    ref_d = _loss_reference(flows64, pc1, pc2, alpha, 1.0, 1.0, 9)
    assert abs(d.item() - ref_d.item()) / abs(ref_d.item()) < 1e-5


# ------------------------------------------------------------------------- train step
def _batch(b, n, seed):
    import synthetic
    return tuple(torch.from_numpy(a).to(DEV) for a in synthetic.ft3d_batch(b, n, seed=seed))[:2]


def test_graphed_selfsup_step_equals_eager():
    """test_gpu_graph.test_graphed_step_equals_eager's train mode without the flow input: the
    same hit / miss prefetch sequence, losses equal as floats, parameters bit for bit."""
    from distill import SelfSupTrainStep, graphed_selfsup_step, make_optimizer
    from models_bid_pointconv import PointConvBidirection
    torch.manual_seed(0)
    base = PointConvBidirection().to(DEV)
    batches = [_batch(2, 2048, s) for s in (1, 2, 3)]
    assert all(len(b) == 2 for b in batches)
    eager_model = copy.deepcopy(base)
    graph_model = copy.deepcopy(base)
    opt_e = make_optimizer(eager_model, capturable=True)
    opt_g = make_optimizer(graph_model, capturable=True)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        eager = SelfSupTrainStep(eager_model, opt_e)
        graphed = graphed_selfsup_step(graph_model, opt_g, batches[0], warmup=1)
    stream_warn = [str(w.message) for w in caught if "AccumulateGrad" in str(w.message)
                   or "stream" in str(w.message).lower()]
    assert not stream_warn, stream_warn
    # the graphed step's constructor ran one eager warm-up step on batches[0]
    eager(*batches[0])
    losses = []
    seq = [(batches[1], batches[2]), (batches[2], batches[0]), (batches[1], None),
           (batches[2], None)]
    for b, nxt in seq:
        le = eager(*b)
        lg = graphed(*b, next_batch=nxt)
        losses.append((float(le), float(lg)))
    torch.cuda.synchronize()
    for le, lg in losses:
        assert math.isfinite(le) and le == lg, losses
    changed = False
    for (name, pe), pg, p0 in zip(eager_model.named_parameters(), graph_model.parameters(),
                                  base.parameters()):
        assert torch.equal(pe, pg), name
        changed = changed or not torch.equal(pe, p0)
    assert changed
