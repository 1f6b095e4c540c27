"""Inference measurements on the MI355X: the full-scan propagation kernel
against the two compositions it replaces, and the graph-replayed predictor against the eager
eval forward.

    python tools/bench_inference.py [--out profiles/inference] [--rounds 5] [--steps a,b,...]

Steps: kernel_b1, kernel_b4 (N = 8192 anchors, 90 000 queries per cloud, C = 3) and
predict_b1, predict_b8 (N = 8192).  Every step runs in a child process of its own under its
own time limit, and the tool stops at the first step that fails or runs out of time.  Within a
step the variants alternate, `--rounds` rounds each; a round times `iters` calls between two
device events after a synchronise; reported: the median round and the min..max spread of the
rounds (repeats of the same code in the same process).  One JSON per step plus summary.json
under --out.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kd-pointcloud_amd"))

STEPS = {"kernel_b1": 240, "kernel_b4": 300, "predict_b1": 420, "predict_b8": 480}  # limits, s
PEAK_F32 = 157.3e12  # f32 VALU peak, FLOP/s
PEAK_HBM = 8.0e12    # bytes/s
N_ANCHORS, N_SCAN = 8192, 90000


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


def kernel_step(b, rounds):
    import torch
    import kdpc_native as K
    import synthetic
    dev = "cuda"
    scans = [torch.from_numpy(synthetic.ft3d_pair(N_SCAN, seed=3, pair=i)[0]).to(dev)
             for i in range(b)]
    g = torch.Generator().manual_seed(0)
    pick = [torch.randperm(N_SCAN, generator=g)[:N_ANCHORS].to(dev) for _ in range(b)]
    anchors = torch.stack([s[i] for s, i in zip(scans, pick)]).contiguous()
    vals = torch.randn(b, N_ANCHORS, 3, generator=g).to(dev)
    dense = torch.stack(scans).contiguous()  # equal lengths: the padded batch is the batch
    qry = dense.reshape(-1, 3)
    offsets = torch.arange(b + 1, dtype=torch.int64, device=dev) * N_SCAN

    def fused():
        return K.flow_propagate(anchors, vals, qry, offsets, N_SCAN)

    def three_nn_blend():
        return K.idw_blend_fwd(anchors, dense, vals, K.three_nn(dense, anchors)[1])[0]

    def knn3_blend():
        return K.idw_blend_fwd(anchors, dense, vals, K.knn_point(3, anchors, dense))[0]

    ref = three_nn_blend()
    same = bool(torch.equal(fused().view_as(ref), ref))
    knn_diff = float((knn3_blend() - ref).abs().max())
    ms = _rounds({"flow_propagate": fused, "three_nn+idw_blend": three_nn_blend,
                  "knn_point(3)+idw_blend": knn3_blend}, rounds, iters=20)
    m = b * N_SCAN
    flops, nbytes = 8.0 * m * N_ANCHORS, 12.0 * m + 12.0 * m + 24.0 * b * N_ANCHORS
    t = statistics.median(ms["flow_propagate"]) * 1e-3
    t_flop, t_mem = flops / PEAK_F32, nbytes / PEAK_HBM
    return {"step": f"kernel_b{b}", "B": b, "N": N_ANCHORS, "queries_per_cloud": N_SCAN, "C": 3,
            "flow_propagate_equals_three_nn_blend": same,
            "knn3_blend_max_abs_diff_vs_three_nn_blend": knn_diff,
            "variants": {k: _stats(v) for k, v in ms.items()},
            "bound": {"distance_evals": float(m) * N_ANCHORS, "flops": flops, "bytes": nbytes,
                      "t_valu_peak_ms": t_flop * 1e3, "t_hbm_peak_ms": t_mem * 1e3,
                      "binds": "f32 VALU" if t_flop >= t_mem else "HBM",
                      "share_of_bound": max(t_flop, t_mem) / t}}


def predict_step(b, rounds):
    import torch
    import synthetic
    from inference import FlowPredictor
    from models_bid_pointconv import PointConvBidirection
    dev = "cuda"
    torch.manual_seed(0)
    model = PointConvBidirection().to(dev).eval()
    batches = []
    for s in (5, 6):
        p1, p2, _ = synthetic.ft3d_batch(b, N_ANCHORS, seed=s)
        batches.append((torch.from_numpy(p1).to(dev), torch.from_numpy(p2).to(dev)))
    eager = FlowPredictor(model, b, N_ANCHORS, graph=False)
    graph = FlowPredictor(model, b, N_ANCHORS)
    graph_pf = FlowPredictor(model, b, N_ANCHORS, prefetch=True)
    want = [eager.predict(*x) for x in batches]
    same = all(bool(torch.equal(graph.predict(*x), w)) for x, w in zip(batches, want))
    turn = [0]

    def run(pred, prefetch=False):
        def fn():
            i = turn[0] = 1 - turn[0]
            kw = {"next_batch": batches[1 - i]} if prefetch else {}
            return pred.predict(*batches[i], **kw)
        return fn
    same_pf = all(bool(torch.equal(run(graph_pf, True)(), want[turn[0]])) for _ in range(4))
    core = model

    def fps_chain():
        with torch.inference_mode():
            return core.precompute_fps(*batches[0])

    def plan():
        with torch.inference_mode():
            return core.precompute_plan(*batches[0], csr=False)
    iters = 20 if b == 1 else 8
    ms = _rounds({"eager": run(eager), "graph": run(graph), "graph+prefetch": run(graph_pf, True),
                  "fps_chain_alone": fps_chain, "coordinate_plan_alone": plan}, rounds, iters)
    # host time per call (enqueue only: what the graph removes)
    host = {}
    for name, pred in (("eager", eager), ("graph", graph)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            pred.predict(*batches[0])
        host[name] = (time.perf_counter() - t0) / iters * 1e3
        torch.cuda.synchronize()
    # latency of one call at a time (synchronise, call, synchronise: host clock), which is
    # what a B = 1 deployment sees; rounds alternate as above
    latency = {"eager": [], "graph": [], "graph+prefetch": []}
    fns = {"eager": run(eager), "graph": run(graph), "graph+prefetch": run(graph_pf, True)}
    for _ in range(rounds):
        for name, fn in fns.items():
            per_call = []
            for _ in range(iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                per_call.append((time.perf_counter() - t0) * 1e3)
            latency[name].append(statistics.median(per_call))
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"step": f"predict_b{b}", "B": b, "N": N_ANCHORS,
            "graph_equals_eager": same, "graph_prefetch_equals_eager": same_pf,
            "variants": {k: _stats(v) for k, v in ms.items()},
            "host_enqueue_ms_per_call": host,
            "latency_one_call_at_a_time": {k: _stats(v) for k, v in latency.items()},
            "fps_chain_share_of_graph_latency": med["fps_chain_alone"] / med["graph"]}


def child(step, rounds, path):
    kind, b = step.split("_b")
    res = (kernel_step if kind == "kernel" else predict_step)(int(b), rounds)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "variants"}))
    for k, v in res["variants"].items():
        print(f"  {k:26s} median {v['median_ms']:.4f} ms  [{v['min_ms']:.4f} .. {v['max_ms']:.4f}]")
    for k, v in res.get("latency_one_call_at_a_time", {}).items():
        print(f"  latency {k:18s} median {v['median_ms']:.4f} ms  "
              f"[{v['min_ms']:.4f} .. {v['max_ms']:.4f}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inference"))
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
