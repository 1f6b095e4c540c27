"""Self-supervised scene-flow loss: Chamfer + flow smoothness over the model's pyramid.

PointPWC-Net's self-supervised objective (Wu et al., ECCV 2020, section 5: the Chamfer and
smoothness terms), for the raw scans that have no flow labels: at every level the first cloud
warped by the predicted flow should lie on the second cloud (Chamfer distance, both
directions) and neighbouring points should move alike (smoothness).  It takes what the model
already returns (flows, pc1, pc2 pyramids) and no ground truth.

  * chamfer_distance -> csrc/chamfer.hip: both directions' nearest neighbours in one launch,
    direct-difference distances (exactly 0 for coincident points anywhere in the scene, where
    knn_point's expanded form cancels); backward = one deterministic kernel per cloud over
    the CSR of the opposite direction's indices (no float atomics).
  * flow_smoothness -> the existing kNN, row gather (CSR backward) and fixed-order sums.
The large sums go through dense.fixed_sum, as in loss_functions.py: reproducible, and
bit-identical between the eager and the graph-replayed step.  No CPU path, as elsewhere.
The third term of PointPWC-Net's loss (Laplacian curvature) is not built.
"""
import torch
from torch.autograd.function import once_differentiable

import kdpc_native as _nat
from dense import fixed_sum
from pointconv_util import index_points_group, knn_point


class _Chamfer(torch.autograd.Function):
    """(a, b) -> (dist_ab, dist_ba, idx_ab, idx_ba); the indices carry no gradient and the
    backward differentiates the distances with the neighbour choices held fixed."""

    @staticmethod
    def forward(ctx, a, b):
        dist_ab, idx_ab, dist_ba, idx_ba = _nat.chamfer_fwd(a, b)
        ctx.save_for_backward(a, b, idx_ab, idx_ba)
        ctx.mark_non_differentiable(idx_ab, idx_ba)
        return dist_ab, dist_ba, idx_ab, idx_ba

    @staticmethod
    @once_differentiable
    def backward(ctx, g_ab, g_ba, _gi_ab, _gi_ba):
        a, b, idx_ab, idx_ba = ctx.saved_tensors
        g_ab, g_ba = g_ab.contiguous(), g_ba.contiguous()
        da = db = None
        # one CSR per cloud that needs a gradient: in training only the warped cloud does
        if ctx.needs_input_grad[0]:
            da = _nat.chamfer_bwd(a, b, idx_ab, g_ab, _nat.csr_of(idx_ba, a.shape[1]), g_ba)
        if ctx.needs_input_grad[1]:
            db = _nat.chamfer_bwd(b, a, idx_ba, g_ba, _nat.csr_of(idx_ab, b.shape[1]), g_ab)
        return da, db


def chamfer_neighbours(a, b):
    """a (B,N,3), b (B,M,3) -> (dist_ab (B,N), dist_ba (B,M), idx_ab (B,N), idx_ba (B,M)):
    chamfer_distance with the (non-differentiable, int32) nearest-neighbour indices."""
    if not a.is_cuda or not b.is_cuda:
        raise _nat.KdpcError("chamfer_distance needs GPU (HIP) tensors: kd-pointcloud_amd has "
                             "no CPU path")
    return _Chamfer.apply(a.contiguous(), b.contiguous())


def chamfer_distance(a, b):
    """a (B,N,3), b (B,M,3) -> (dist_ab (B,N), dist_ba (B,M)): every point's squared distance
    to its nearest point of the other cloud (the lower index on ties), differentiable in a
    and b."""
    return chamfer_neighbours(a, b)[:2]


def flow_smoothness(pc, flow, k=9):
    """PointPWC-Net's smoothness term: mean_b sum_n sum_k ||flow[idx[n,k]] - flow[n]|| / (k-1)
    over each point's k nearest points of pc (itself among them: a zero difference, whose
    norm has gradient 0).  pc, flow (B,N,3) point-major."""
    B, N, _ = flow.shape
    idx = knn_point(k, pc, pc)
    diff = index_points_group(flow, idx) - flow.reshape(B, N, 1, 3)
    per_point = fixed_sum(torch.norm(diff, dim=3), 2) / (k - 1)
    return fixed_sum(per_point, 1).mean()


def multiScaleChamferSmooth(pred_flows, pc1, pc2, alpha=[0.02, 0.04, 0.08, 0.16], f_chamfer=1.0,
                            f_smooth=1.0, k_smooth=9):
    """sum_i alpha_i (f_chamfer (chamfer(pc1_i + flow_i, pc2_i)) + f_smooth smoothness_i) over
    the levels of pred_flows; pred_flows[i], pc1[i], pc2[i] are the (B,3,N_i) views the model
    returns.  The weights are PointPWC-Net's.  Returns a (1,) tensor like multiScaleLoss."""
    total_loss = torch.zeros(1, device=pred_flows[0].device, dtype=pred_flows[0].dtype)
    for i in range(len(pred_flows)):
        p1 = pc1[i].permute(0, 2, 1).contiguous()
        flow = pred_flows[i].permute(0, 2, 1)
        warp = p1 + flow
        dist_ab, dist_ba = chamfer_distance(warp, pc2[i].permute(0, 2, 1))
        chamfer = fixed_sum(dist_ab, 1).mean() + fixed_sum(dist_ba, 1).mean()
        smooth = flow_smoothness(p1, flow, k_smooth)
        total_loss += alpha[i] * (f_chamfer * chamfer + f_smooth * smooth)
    return total_loss
