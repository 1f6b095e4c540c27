"""GPU: the ranked cost-volume backward skips the neighbour rows no output routes to.

A (query, neighbour) row that no output's argmax points at has dz0 = d(dir) = +0 exactly, so
kdpc_cost_volume_bwd_csr neither writes its dP2 row to the CSR workspace nor reads it back in
the row sum (the .w of the row's d(dir) float4 is the flag).  The reference everywhere is the
plain entry point, kdpc_cost_volume_bwd followed by kdpc_group_rows_grad through the CSR, which
writes every row and knows nothing of flags: all five outputs must be torch.equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ["dp1", "dp2", "dx1", "dx2", "dparams"]


def _inputs(din, dout, n1, n2, bsz, k, seed, idx=None, boost=True):
    """Inputs as tests/test_gpu_fused.py::test_cost_volume_bwd_csr_bitwise builds them; with
    `boost`, the P2 rows of a seeded random quarter of the reference points are multiplied by
    4, which concentrates the max on some neighbours."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x1 = torch.rand(bsz, n1, 3, generator=g)
    x2 = torch.rand(bsz, n2, 3, generator=g)
    ridx = torch.randint(0, n2 - 1, (bsz, n1, k), generator=g, dtype=torch.int32)
    p1 = torch.randn(bsz, n1, din, generator=g)
    p2 = torch.randn(bsz, n2, din, generator=g)
    wpos = torch.randn(din, 3, generator=g) * 0.3
    bpos = torch.randn(din, generator=g) * 0.1
    w1 = torch.randn(dout, din, generator=g) / din ** 0.5
    b1 = torch.randn(dout, generator=g) * 0.1
    gout = torch.randn(bsz, n1, dout, generator=g)
    if boost:
        hot = torch.rand(bsz, n2, generator=g) < 0.25
        p2 = torch.where(hot[..., None], p2 * 4, p2)
    idx = ridx if idx is None else idx
    return [t.to(DEV).contiguous() for t in (x1, x2, idx, p1, p2, wpos, bpos, w1, b1, gout)]


def _live(amax, k):
    """(B, N1, K) bool: some output's argmax is that neighbour row."""
    bsz, n1, _ = amax.shape
    live = torch.zeros(bsz, n1, k, dtype=torch.bool, device=amax.device)
    return live.scatter_(2, amax.long(), True)


def _reference(K, x1, x2, idx, p1, p2, wpos, bpos, w1, out, amax, gout):
    bsz, n1, k = idx.shape
    n2, din = x2.shape[1], p1.shape[2]
    dp1, dp2r, dx1, ddr, dpar = K.cost_volume_bwd(x1, x2, idx, p1, p2, wpos, bpos, w1, out, amax,
                                                  gout)
    csr = K.csr_of(idx, n2)
    dp2 = K.group_rows_grad(dp2r.view(bsz, n1 * k, din), csr, bsz, n2, din)
    dx2 = K.group_rows_grad(ddr.view(bsz, n1 * k, 3), csr, bsz, n2, 3)
    return [dp1, dp2, dx1, dx2, dpar]


def _check(K, x1, x2, idx, p1, p2, wpos, bpos, w1, out, amax, gout, slope0=False):
    """The ranked entry point against the reference, bit for bit; reference points that
    receive no live row (none at all, or dead rows only) get exact zeros.  Returns the live
    fraction of the (n, k) rows."""
    ref = _reference(K, x1, x2, idx, p1, p2, wpos, bpos, w1, out, amax, gout)
    args = (x1, x2, idx, p1, p2, wpos, bpos, w1, out, amax, gout)
    runs = [("ranked", K.cost_volume_bwd_csr(*args))]
    if slope0:
        bsz, n1, k = idx.shape
        z = torch.zeros(bsz, n1, k, p1.shape[2], dtype=torch.uint8, device=DEV)
        runs.append(("slope0", K.cost_volume_bwd_csr(*args, slope0=z)))
    for tag, r in runs:
        for name, a, b in zip(NAMES, r, ref):
            assert a.shape == b.shape and torch.equal(a, b), (tag, name)
    bsz, n1, k = idx.shape
    n2 = x2.shape[1]
    live = _live(amax, k)
    hits = torch.zeros(bsz, n2, device=DEV).scatter_add_(
        1, idx.view(bsz, -1).long(), live.view(bsz, -1).float())
    none = hits == 0
    assert none.any()
    r = runs[0][1]
    assert torch.count_nonzero(r[1][none]) == 0 and torch.count_nonzero(r[3][none]) == 0
    return float(live.float().mean())


SHAPES = [(32, 32, 1000, 900, 2, 32), (64, 64, 513, 700, 3, 32), (32, 64, 300, 300, 1, 17),
          (64, 32, 257, 600, 2, 9), (128, 128, 300, 280, 2, 32), (256, 256, 200, 250, 2, 20)]


@pytest.mark.parametrize("din,dout,n1,n2,bsz,k", SHAPES)
def test_dead_rows_bitwise(din, dout, n1, n2, bsz, k):
    """Both kinds of row in every case (between 5 % and 95 % of the rows are dead), with and
    without an all-zero slope0; the last point of each cloud is picked by no query."""
    import kdpc_native as K
    x1, x2, idx, p1, p2, wpos, bpos, w1, b1, gout = _inputs(din, dout, n1, n2, bsz, k,
                                                            din * 7 + k)
    out, amax = K.cost_volume_fwd(x1, x2, idx, p1, p2, wpos, bpos, w1, b1)
    frac = _check(K, x1, x2, idx, p1, p2, wpos, bpos, w1, out, amax, gout, slope0=True)
    print(f"live fraction {frac:.3f}")
    assert 0.05 <= 1.0 - frac <= 0.95, frac


@pytest.mark.parametrize("din,dout,k", [(32, 32, 32), (64, 64, 32), (32, 64, 17), (128, 128, 32),
                                        (256, 256, 20)])
def test_all_routing_to_one_row(din, dout, k):
    """One overwhelmingly large P2 row, first in every idx row, under a positive W1: every
    output of every query routes to neighbour 0, one live row of k.  Every other reference
    point receives dead rows only (or none: the last but one) and gets exact zeros."""
    import kdpc_native as K
    n1, n2, bsz = 150, 120, 2
    x1, x2, idx, p1, p2, wpos, bpos, w1, b1, gout = _inputs(din, dout, n1, n2, bsz, k, 11 + din,
                                                            boost=False)
    idx = idx.clamp(max=n2 - 3).contiguous()  # n2 - 2: no query picks it
    idx[:, :, 0] = n2 - 1
    p2[:, n2 - 1] = 1000.0
    w1 = w1.abs().contiguous()
    out, amax = K.cost_volume_fwd(x1, x2, idx, p1, p2, wpos, bpos, w1, b1)
    assert int(amax.max()) == 0
    frac = _check(K, x1, x2, idx, p1, p2, wpos, bpos, w1, out, amax, gout)
    assert abs(frac - 1.0 / k) < 1e-6
    r = K.cost_volume_bwd_csr(x1, x2, idx, p1, p2, wpos, bpos, w1, out, amax, gout)
    assert torch.count_nonzero(r[1][:, :n2 - 1]) == 0 and torch.count_nonzero(r[3][:, :n2 - 1]) == 0
    assert torch.count_nonzero(r[1][:, n2 - 1]) > 0


@pytest.mark.parametrize("din,dout,k", [(32, 64, 1), (64, 64, 1), (32, 64, 4), (64, 64, 4)])
def test_every_row_live(din, dout, k):
    """Output o routes to row o % k: with D_OUT = 64 >= k no row is dead."""
    import kdpc_native as K
    n1, n2, bsz = 200, 150, 2
    x1, x2, idx, p1, p2, wpos, bpos, w1, b1, gout = _inputs(din, dout, n1, n2, bsz, k, 23 + k)
    out, _ = K.cost_volume_fwd(x1, x2, idx, p1, p2, wpos, bpos, w1, b1)
    amax = (torch.arange(dout, device=DEV) % k).to(torch.uint8).expand(bsz, n1, dout).contiguous()
    frac = _check(K, x1, x2, idx, p1, p2, wpos, bpos, w1, out, amax, gout)
    assert frac == 1.0


@pytest.mark.parametrize("routing", ["concentrated", "random"])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_segment_longer_than_one_window(d, routing):
    """Every neighbour of every query is one reference point: its segment of 64 * 32 = 2048
    rows spans several LDS windows of the row sum (455 rows at D = 32, 240 at D = 64, 124 at
    D = 128).  The neighbour rows of a query are then identical, so any argmax is a valid
    forward result: all zeros (one live row per query) and seeded random rows."""
    import kdpc_native as K
    n1, n2, bsz, k = 64, 8, 2, 32
    one = torch.full((bsz, n1, k), 3, dtype=torch.int32)
    x1, x2, idx, p1, p2, wpos, bpos, w1, b1, gout = _inputs(d, d, n1, n2, bsz, k, 5 + d, idx=one)
    out, amax = K.cost_volume_fwd(x1, x2, idx, p1, p2, wpos, bpos, w1, b1)
    amax = torch.zeros_like(amax)
    if routing == "random":
        g = torch.Generator(device="cpu").manual_seed(d)
        amax = torch.randint(0, k, (bsz, n1, d), generator=g).to(torch.uint8).to(DEV)
        amax[:, ::7] = 5  # and some queries with a single live row in between
    frac = _check(K, x1, x2, idx, p1, p2, wpos, bpos, w1, out, amax, gout)
    assert (frac == 1.0 / k) if routing == "concentrated" else (0.3 < frac < 0.99)


@pytest.mark.parametrize("din,dout,n1,n2,bsz,k", [SHAPES[1], SHAPES[4]])
def test_stale_workspace(din, dout, n1, n2, bsz, k):
    """The C entry point with a caller-owned workspace full of NaN: the slots of dead rows are
    never written, so they stay NaN and must not reach the sums."""
    import kdpc_native as K
    x1, x2, idx, p1, p2, wpos, bpos, w1, b1, gout = _inputs(din, dout, n1, n2, bsz, k,
                                                            din * 7 + k)
    out, amax = K.cost_volume_fwd(x1, x2, idx, p1, p2, wpos, bpos, w1, b1)
    ref = _reference(K, x1, x2, idx, p1, p2, wpos, bpos, w1, out, amax, gout)
    csr = K.csr_rank_of(idx, n2)
    nbytes = K.load_library().kdpc_cost_volume_bwd_csr_workspace_bytes(bsz, n1, k, din, dout)
    assert nbytes > 0
    nan = float("nan")
    ws = torch.full(((nbytes + 3) // 4,), nan, device=DEV)
    res = [torch.full_like(t, nan) for t in ref]
    dp1, dp2, dx1, dx2, dpar = res
    K._call("kdpc_cost_volume_bwd_csr", bsz, n1, n2, k, din, dout, x1.data_ptr(), x2.data_ptr(),
            idx.data_ptr(), p1.data_ptr(), p2.data_ptr(), wpos.data_ptr(), bpos.data_ptr(),
            w1.data_ptr(), out.data_ptr(), amax.data_ptr(), None, gout.data_ptr(),
            csr.offsets.data_ptr(), csr.rank.data_ptr(), dp1.data_ptr(), dp2.data_ptr(),
            dx1.data_ptr(), dx2.data_ptr(), ws.data_ptr(), nbytes, dpar.data_ptr(),
            K._stream(x1))
    torch.cuda.synchronize()
    assert torch.isnan(ws).any()  # dead slots were left alone
    for name, a, b in zip(NAMES, res, ref):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), name
