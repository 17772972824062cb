"""What a 3129-label answer head (the reference's `vqa` task) costs next to the 100-label one, in one process on one GPU:
  1. the 12-layer B = 32 384 x 384 DAT train_step (default fp16 engine, hipGraph replay) at C = 100 and C = 3129: ms / step,
     and the launches of the serial tail whose size depends on C, each timed alone (warm, HIP events around 20 back-to-back
     launches);
  2. the any-width loss feddat_dat_loss_fwd_bwd_wide alone at (32, 3129), 20 launches captured in one hipGraph, next to the
     two-launch feddat_dat_loss_fwd_bwd on the same inputs (five repetitions each, interleaved; the spread is max - min of the
     five);
  3. the single-workgroup BCE feddat_bce_loss_fwd_bwd (optimizer_mode adapter / bias / norm) at (32, 3129), the same way.
python tools/wide_head_bench.py [--skip-step]     (output kept in profiles/wide_head_bench.txt)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from feddat_amd import engine, lib as L, vilt_spec

dev = torch.device("cuda", 0)
H, B = 768, 32
REPS, LAUNCHES = 5, 20


def timed(fn, n=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n       # us per call


def graph_of(fn, launches=LAUNCHES):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def report(name, ts):
    print(f"{name:58s} median {statistics.median(ts):8.2f} us   min {min(ts):8.2f}   max {max(ts):8.2f}   spread {max(ts) - min(ts):6.2f}")


def step_and_tail(C):
    params = vilt_spec.random_init(12, ["c0"], seed=0, num_labels=C)
    e = engine.ViltDatEngine(params, ["c0"], dev, batch=B, res=384, layers=12, num_labels=C)
    batches = [vilt_spec.synthetic_batch(B, 384, 1234 + i, device=dev, num_labels=C) for i in range(4)]
    e.begin_local_update("c0", steps_per_epoch=80)
    for i in range(4):
        e.train_step(batches[i], use_graph=True)
    torch.cuda.synchronize()
    ts = [timed(lambda: e.train_step(None, use_graph=True), 10) / 1e3 for _ in range(REPS)]
    print(f"C = {C:4d}: DAT train_step, 12 layers, B = 32, 384 x 384, fp16 operands, hipGraph: median {statistics.median(ts):.3f} ms/step "
          f"(min {min(ts):.3f}, max {max(ts):.3f}); loss_0 {float(e._loss_tensor()[0]):.3f}")
    hp, pre = e.head["c0"], "task_layer.c0."
    with L.operands(e.operands):
        J = L.ht_job
        W1, b1 = hp.view(pre + "clf_fc1.weight"), hp.view(pre + "clf_fc1.bias")
        dW1, db1 = hp.view(pre + "clf_fc1.weight", hp.g), hp.view(pre + "clf_fc1.bias", hp.g)
        s, s2 = e.hd["both"], e.hd["p2"]
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        dl = e.dlogits

        def loss():
            if C > 128:
                L.dat_loss_fwd_bwd_wide(s["logits"][B:], s["logits"][:B], e.inp["target"], dl, e.loss_buf["p1"], e.loss_ws,
                                        nonfinite=flag)
            else:
                L.dat_loss_fwd_bwd_checked(s["logits"][B:], s["logits"][:B], e.inp["target"], dl, e.loss_buf["p1"], flag)
        tail = {
            f"fc1, 2B rows (64 x {C} x 1536)": lambda: L.head_gemm(J(s["g0"], 2 * H, 1, W1, 1, 2 * H, 2 * B, C, 2 * H, s["logits"], bias_j=b1)),
            f"fc1, B rows (32 x {C} x 1536)": lambda: L.head_gemm(J(s2["g0"], 2 * H, 1, W1, 1, 2 * H, B, C, 2 * H, s2["logits"], bias_j=b1)),
            ("DAT loss (feddat_dat_loss_fwd_bwd_wide + flag)" if C > 128 else "DAT loss (feddat_dat_loss_fwd_bwd_checked)"): loss,
            f"dW_fc1 ({C} x 1536 x 32) | dn0 (32 x 1536 x {C})": lambda: L.head_gemm(
                J(dl, 1, C, s2["g0"], 2 * H, 1, C, 2 * H, B, dW1, mode=1, colsum=db1),
                J(dl, C, 1, W1, 2 * H, 1, B, 2 * H, C, e.dn0, epi=L.HT_EPI_MUL_DGELU, aux=s2["n0"], ld_aux=2 * H)),
            f"  dW_fc1 alone (K = 32)": lambda: L.head_gemm(J(dl, 1, C, s2["g0"], 2 * H, 1, C, 2 * H, B, dW1, mode=1, colsum=db1)),
            f"  dn0 alone (K = {C}{'' if C % 4 == 0 else ', K % 4 != 0'})": lambda: L.head_gemm(
                J(dl, C, 1, W1, 2 * H, 1, B, 2 * H, C, e.dn0, epi=L.HT_EPI_MUL_DGELU, aux=s2["n0"], ld_aux=2 * H)),
            f"AdamW, head alone ({hp.p.numel()} floats)": lambda: e._adamw_many([e._adamw_group(hp)]),
        }
        for name, fn in tail.items():
            fn()
            torch.cuda.synchronize()
            report(f"  C = {C:4d} {name}", [timed(fn, LAUNCHES) for _ in range(REPS)])
    del e
    torch.cuda.empty_cache()


def losses_alone(Bn=32, C=3129):
    g = torch.Generator().manual_seed(0)
    x, t = (torch.randn(Bn, C, generator=g) * 2).to(dev), (torch.randn(Bn, C, generator=g) * 2).to(dev)
    y = vilt_spec.synthetic_batch(Bn, 32, 5, num_labels=C)["target_scores"].to(dev)
    dl, sc = torch.empty(Bn, C, device=dev), torch.empty(4 + 2 * Bn, device=dev)
    ws = torch.empty(L.dat_loss_wide_workspace_elems(Bn), device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    cases = {
        "feddat_dat_loss_fwd_bwd_wide (+ flag)": lambda: L.dat_loss_fwd_bwd_wide(x, t, y, dl, sc, ws, nonfinite=flag),
        "feddat_dat_loss_fwd_bwd (two launches, one wave per row)": lambda: L.dat_loss_fwd_bwd(x, t, y, dl, sc),
        "feddat_bce_loss_fwd_bwd (one workgroup)": lambda: L.bce_loss_fwd_bwd(x, y, dl, sc, flag),
    }
    graphs = {n: graph_of(f) for n, f in cases.items()}
    ts = {n: [] for n in cases}
    for _ in range(REPS):
        for n, gr in graphs.items():
            for _ in range(3):
                gr.replay()
            ts[n].append(timed(gr.replay, 5) / LAUNCHES)
    print(f"losses alone at ({Bn}, {C}): us per call inside a hipGraph of {LAUNCHES} calls, {REPS} repetitions")
    for n in cases:
        report("  " + n, ts[n])
    w, o = ts["feddat_dat_loss_fwd_bwd_wide (+ flag)"], ts["feddat_dat_loss_fwd_bwd (two launches, one wave per row)"]
    spread = max(max(w) - min(w), max(o) - min(o))
    print(f"  wide - two-launch (medians): {statistics.median(w) - statistics.median(o):+.2f} us; spread between repetitions {spread:.2f} us")


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0))
    with L.operands("f16"):
        losses_alone()
    if "--skip-step" not in sys.argv:
        for C in (100, 3129):
            step_and_tail(C)
