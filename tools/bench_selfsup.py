"""Self-supervised training measurements on the MI355X: the fused Chamfer
kernels against the composition of existing ops they replace, and the graphed self-supervised
step against the graphed supervised step.

    python tools/bench_selfsup.py [--out profiles/selfsup] [--rounds 5] [--steps a,b,...]

Steps: chamfer (the four pyramid sizes N = M = 8192, 2048, 512, 256 at B = 8; variants:
`chamfer_fwd` against three_nn both ways, and `chamfer_fwd + chamfer_bwd` through
selfsup.chamfer_distance against three_nn both ways + torch gathers with their index_add
backward, both differentiating the same summed distances with respect to the first cloud) and
step_b8 (distill.graphed_selfsup_step against distill.graphed_flow_step at B = 8, N = 8192).
Every step runs in a child process of its own under its own time limit, and the tool stops at
the first step that fails or runs out of time.  Within a step the variants alternate,
`--rounds` rounds each; a round times `iters` calls between two device events after a
synchronise; reported: the median round and the min..max spread of the rounds.  One JSON per
step plus summary.json under --out.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kd-pointcloud_amd"))

STEPS = {"chamfer": 300, "step_b8": 480}  # limits, s
PEAK_F32 = 157.3e12  # f32 VALU peak, FLOP/s
PEAK_HBM = 8.0e12    # bytes/s
LEVELS = (8192, 2048, 512, 256)
BATCH = 8


def _rounds(variants, rounds, iters):
    """variants: {name: fn}.  -> {name: [ms per call, one per round]}, variants alternating."""
    import torch
    out = {k: [] for k in variants}
    for fn in variants.values():  # warm up every variant at the timed shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / iters)
    return out


def _stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "rounds_ms": ms}


def _rows(x, idx):
    return x.gather(1, idx.long()[..., None].expand(-1, -1, 3))


def chamfer_level(n, rounds):
    import torch
    import kdpc_native as K
    import selfsup
    import synthetic
    dev = "cuda"
    p1, p2, flow = synthetic.ft3d_batch(BATCH, n, seed=4)
    # a converging model's situation: the warped cloud a few centimetres off the second one
    g = torch.Generator().manual_seed(n)
    a = (torch.from_numpy(p1 + flow) + 0.02 * torch.randn(BATCH, n, 3, generator=g)).to(dev)
    b = torch.from_numpy(p2).to(dev)
    a_req = a.clone().requires_grad_()

    def fused_fwd():
        return K.chamfer_fwd(a, b)

    def composed_fwd():
        d_ab, i_ab = K.three_nn(a, b)
        d_ba, i_ba = K.three_nn(b, a)
        return d_ab[..., 0], i_ab[..., 0], d_ba[..., 0], i_ba[..., 0]

    def fused_fwd_bwd():
        a_req.grad = None
        d_ab, d_ba = selfsup.chamfer_distance(a_req, b)
        (d_ab.sum() + d_ba.sum()).backward()
        return a_req.grad

    def composed_fwd_bwd():
        a_req.grad = None
        with torch.no_grad():
            i_ab = K.three_nn(a_req, b)[1][..., 0]
            i_ba = K.three_nn(b, a_req)[1][..., 0]
        d_ab = ((a_req - _rows(b, i_ab)) ** 2).sum(-1)
        d_ba = ((b - _rows(a_req, i_ba)) ** 2).sum(-1)
        (d_ab.sum() + d_ba.sum()).backward()
        return a_req.grad

    same = all(bool(torch.equal(x, y.contiguous())) for x, y in zip(fused_fwd(), composed_fwd()))
    gf, gc = fused_fwd_bwd().clone(), composed_fwd_bwd().clone()
    grad_diff = float((gf - gc).abs().max() / gc.abs().max())
    iters = 50 if n <= 2048 else 20
    ms = _rounds({"chamfer_fwd": fused_fwd, "three_nn x2": composed_fwd,
                  "chamfer_fwd+bwd": fused_fwd_bwd,
                  "three_nn x2 + gather/index_add": composed_fwd_bwd}, rounds, iters)
    evals = 2.0 * BATCH * n * n
    flops, nbytes = 8.0 * evals, 2.0 * BATCH * n * (12 + 12 + 8)
    t = statistics.median(ms["chamfer_fwd"]) * 1e-3
    t_flop, t_mem = flops / PEAK_F32, nbytes / PEAK_HBM
    return {"B": BATCH, "N": n, "M": n, "forward_equals_three_nn_first_column": same,
            "grad_max_abs_diff_over_max_grad_vs_composition": grad_diff,
            "variants": {k: _stats(v) for k, v in ms.items()},
            "bound": {"distance_evals": evals, "flops": flops, "bytes": nbytes,
                      "t_valu_peak_ms": t_flop * 1e3, "t_hbm_peak_ms": t_mem * 1e3,
                      "binds": "f32 VALU" if t_flop >= t_mem else "HBM",
                      "share_of_bound": max(t_flop, t_mem) / t}}


def chamfer_step(rounds):
    return {"step": "chamfer", "levels": {str(n): chamfer_level(n, rounds) for n in LEVELS}}


def train_step(rounds):
    import copy
    import torch
    import synthetic
    from distill import graphed_flow_step, graphed_selfsup_step, make_optimizer
    from models_bid_pointconv import PointConvBidirection
    dev = "cuda"
    torch.manual_seed(0)
    base = PointConvBidirection().to(dev)
    batches = [tuple(torch.from_numpy(x).to(dev) for x in synthetic.ft3d_batch(BATCH, 8192, seed=s))
               for s in (5, 6)]
    m_sup, m_self = copy.deepcopy(base), copy.deepcopy(base)
    sup = graphed_flow_step(m_sup, make_optimizer(m_sup, capturable=True), batches[0])
    slf = graphed_selfsup_step(m_self, make_optimizer(m_self, capturable=True), batches[0][:2])
    turn = [0]

    def run(step, k):
        def fn():
            i = turn[0] = 1 - turn[0]
            return step(*batches[i][:k], next_batch=batches[1 - i][:k])
        return fn
    ms = _rounds({"graphed_flow_step (supervised)": run(sup, 3),
                  "graphed_selfsup_step": run(slf, 2)}, rounds, iters=10)
    losses = {"supervised": float(run(sup, 3)()), "selfsup": float(run(slf, 2)())}
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"step": "step_b8", "B": BATCH, "N": 8192, "last_loss": losses,
            "variants": {k: _stats(v) for k, v in ms.items()},
            "selfsup_over_supervised": med["graphed_selfsup_step"] /
            med["graphed_flow_step (supervised)"]}


def _print_variants(variants, indent="  "):
    for k, v in variants.items():
        print(f"{indent}{k:34s} median {v['median_ms']:.4f} ms  "
              f"[{v['min_ms']:.4f} .. {v['max_ms']:.4f}]")


def child(step, rounds, path):
    res = chamfer_step(rounds) if step == "chamfer" else train_step(rounds)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    if step == "chamfer":
        for n, lv in res["levels"].items():
            print(json.dumps({k: v for k, v in lv.items() if k != "variants"}))
            _print_variants(lv["variants"])
    else:
        print(json.dumps({k: v for k, v in res.items() if k != "variants"}))
        _print_variants(res["variants"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selfsup"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3")
    os.makedirs(args.out, exist_ok=True)
    if args.child:
        return child(args.child, args.rounds, os.path.join(args.out, args.child + ".json"))
    summary = {}
    for step in args.steps.split(","):
        if step not in STEPS:
            ap.error(f"unknown step {step!r}")
        print(f"== {step} (limit {STEPS[step]} s)", flush=True)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step,
                                "--rounds", str(args.rounds), "--out", args.out],
                               timeout=STEPS[step])
        except subprocess.TimeoutExpired:
            print(f"{step}: time limit of {STEPS[step]} s reached; stopping", flush=True)
            return 124
        if r.returncode != 0:
            print(f"{step}: failed with exit status {r.returncode}; stopping", flush=True)
            return r.returncode if r.returncode > 0 else 1
        with open(os.path.join(args.out, step + ".json")) as f:
            summary[step] = json.load(f)
    with open(os.path.join(args.out, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
