#!/usr/bin/env python
"""BiImageBertForSequenceClassificationPlus.fuse_head, forward + backward, against the torch composition of the same head
(torch.cat / F.dropout / F.linear / relu on the same parameters) in one process: B = 64, H = 768, dropout 0.1, training mode,
  vqa  num_labels 3129, classifier "mlp"     (the per-GPU batch of BASELINE.json configs[4])
  ve   num_labels 3,    classifier "linear"
Paired, alternating windows (each window: ITERS forward + backward passes between two device events); medians, spreads
(min .. max of the windows) and kernel launches per pass (torch.profiler) -> profiles/r08_plus_head.json.

Run on the GPU:  python tools/bench_plus_head.py [--out profiles/r08_plus_head.json]
Kernel time of one side alone (a run of its own under `rocprofv3 --kernel-trace --stats`; total over 20 + WINDOWS * ITERS passes):
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_plus_head.py --forms vqa --only fused \
      --windows 1 --iters 80 --no-launches --out DIR/ignored.json
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_util as gu  # noqa: E402
from mvp_pytorch_amd import modeling  # noqa: E402

B, WINDOWS, ITERS = 64, 15, 200
FORMS = {"vqa": dict(num_labels=3129, classifier="mlp", loss_type="bce"), "ve": dict(num_labels=3, classifier="linear", loss_type="ce")}


def torch_head(model, pooled, gt, gi):
    p, tr = model.dropout.p, model.training

    def mlp(seq, x):
        if isinstance(seq, torch.nn.Sequential):
            return F.linear(torch.relu(F.linear(x, seq[0].weight, seq[0].bias)), seq[2].weight, seq[2].bias)
        return F.linear(x, seq.weight, seq.bias)
    single = mlp(model.single_mapping, F.dropout(torch.cat([gt, gi, gi - gt, gi * gt], 1), p, tr))
    return mlp(model.classifier, F.dropout(torch.cat([pooled, single], 1), p, tr))


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us per pass


def launches(fn):
    """Kernel launches of one pass, or None when the profiler is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception as exc:       # the measurement stays usable without the count
        print("launch count unavailable:", repr(exc))
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_plus_head.json"))
    ap.add_argument("--no-launches", action="store_true")
    ap.add_argument("--forms", default="vqa,ve")
    ap.add_argument("--only", choices=["both", "fused", "torch"], default="both", help="time one side alone (kernel traces)")
    ap.add_argument("--windows", type=int, default=WINDOWS)
    ap.add_argument("--iters", type=int, default=ITERS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_plus_head needs an MI355X"
    dev = torch.device("cuda:0")
    result = {"B": B, "H": gu.BASE_CFG["hidden_size"], "dropout": 0.1, "windows": args.windows, "iters_per_window": args.iters,
              "unit": "us per forward + backward pass of the head", "forms": {},
              "note": "device events around ITERS eager passes: host launch time included; no gradient arena (SmallLinearFn allocates and zero-fills its weight / bias gradient buffers)"}
    for tag in args.forms.split(","):
        extra = FORMS[tag]
        cfg = dict(gu.BASE_CFG, num_hidden_layers=2, vocab_size=1200, only_word_size=1000, max_position_embeddings=64,
                   hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, **extra)     # the head only depends on H
        torch.manual_seed(0)
        model = modeling.BiImageBertForSequenceClassificationPlus(modeling.make_config(cfg)).to(dev).train()
        H = cfg["hidden_size"]
        ins = [torch.randn(B, H, device=dev, requires_grad=True) for _ in range(3)]
        dy = torch.randn(B, cfg["num_labels"], device=dev)
        params = [p for n, p in model.named_parameters() if n.startswith(("single_mapping.", "classifier."))]

        def run(head):
            for t in ins + params:
                t.grad = None
            head(model, *ins).backward(dy)

        fused = lambda: run(lambda m, *x: m.fuse_head(*x))  # noqa: E731
        composed = lambda: run(torch_head)  # noqa: E731
        sides = [(n, fn) for n, fn in (("fused", fused), ("torch", composed)) if args.only in ("both", n)]
        for _, fn in sides:                   # warm at the timed shape
            window(fn, 20)
        times = {n: [] for n, _ in sides}
        for _ in range(args.windows):         # paired, alternating
            for n, fn in sides:
                times[n].append(window(fn, args.iters))
        form = {n + "_us": {"median": statistics.median(t), "min": min(t), "max": max(t)} for n, t in times.items()}
        if args.only == "both":
            form["paired_ratio_fused_over_torch_median"] = statistics.median(f / c for f, c in zip(times["fused"], times["torch"]))
        result["forms"][tag] = dict(extra, **form)
        print(tag, json.dumps(form), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
        if not args.no_launches and args.only == "both":
            form["launches"] = {"fused": launches(fused), "torch": launches(composed)}
            print(tag, "launches", form["launches"], flush=True)
            result["forms"][tag] = dict(extra, **form)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
