#!/usr/bin/env python
"""Round 7: variable-length batches through train.GraphedStep, today's path against bucket=True, in ONE process.

Headline shape (BERT-base two-stage model, B = 256, T 70 / P 5 / G 20 / R 50, dropout 0.1, clip 10.0, AdamW in the step); eight
synthetic batches with eight different sets of counts are cycled through the timed loop, every step on freshly copied device
tensors (pinned host copies, non_blocking), as a data loader delivers them.  Two legs, alternated and repeated (the machines of
a pool differ by several per cent: only a pair measured in one run means anything):
  (a) exact   GraphedStep(bucket=None): its four graphs are taken by four OTHER batches first (what the first batches of a data
              loader do to it), so the eight timed batches run eagerly — the state of a production job after a few steps;
  (b) bucket  GraphedStep(bucket=True): bounded uni-modal passes, one graph (two at most) for all eight.
Per leg and repeat: ms per step from device events over --steps steps, host ms to queue ONE step behind an empty queue (median of
three; the method of bench.py), and the stepper's capture / replay / eager counters.  Writes --out (JSON).

--launches LEG: no timing; LEG in {exact, bucket} steps one model eagerly --steps times on the eight batches (graphs off), for a
`rocprofv3 --kernel-trace --stats -- python tools/varlen_graph_bench.py --launches LEG` run that counts the launches per step.

Needs a GPU:  python tools/varlen_graph_bench.py [--batch 256] [--steps 40] [--repeats 3]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from mvp_pytorch_amd import dp, engine, hip, modeling, train  # noqa: E402
from mvp_pytorch_amd.modeling.modeling_vlbert import BOUND_KEYS  # noqa: E402
from mvp_pytorch_amd.synthetic import synthetic_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--seeds", type=int, default=8)
ap.add_argument("--launches", choices=["exact", "bucket"], default=None)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r07_varlen_graph.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("varlen_graph_bench: needs an MI355X")
dev = torch.device("cuda:0")
hip.load()
dims = dict(B=args.batch, T=70, P=5, G=20, R=50)
cfg = bench.BASE_CFG


def host_batch(seed):
    b = synthetic_batch(dims, cfg, seed)
    return {k: (v.pin_memory() if torch.is_tensor(v) else v) for k, v in b.items()}


def fresh(hb):
    return {k: (v.to(dev, non_blocking=True) if torch.is_tensor(v) else v) for k, v in hb.items()}


pool = [host_batch(s) for s in range(args.seeds)]
counts = [tuple(int(b["host_counts"][k]) for k in train.COUNT_KEYS) for b in pool]
assert len(set(counts)) == len(pool), "the batches must differ in their counts"


def make_leg(bucket, graphed=True):
    torch.manual_seed(1234)
    engine._seed_counter[0] = 0x5DEECE66D
    model = modeling.BiBertImgForPreTraining(modeling.make_config(cfg)).to(dev).train()
    opt, sched = train.build_optimizer(model, lr=5e-5, adam_epsilon=1e-8, weight_decay=0.01, t_total=100000)
    sync = dp.GradSync(model)
    step = train.GraphedStep(model, opt, sched, max_tag_length=dims["G"], max_grad_norm=10.0, grad_sync=sync, bucket=bucket, enabled=graphed)
    return dict(step=step, sync=sync, model=model, n=0)


def run_steps(leg, n):
    loss = None
    for _ in range(n):
        loss = leg["step"](fresh(pool[leg["n"] % len(pool)]))
        leg["n"] += 1
    return loss


if args.launches:
    leg = make_leg(None, graphed=False)
    if args.launches == "bucket":           # the bounded path, eagerly: the stepper's own bounds, attached by hand
        caps = train.batch_caps(pool[0])
        known = []
        for hb, c in zip(pool, counts):
            bounds, _ = train.cover_bounds(known, c, caps, train.bucket_quanta(True))
            hb["host_counts"] = type(hb["host_counts"])(hb["host_counts"], **dict(zip(BOUND_KEYS, bounds)))
    run_steps(leg, args.steps)
    torch.cuda.synchronize()
    hip.check_device_errors(dev)
    print("launches leg %s: %d eager steps (divide the trace's dispatch count by this; the first step also makes the weight copies)" % (args.launches, args.steps))
    leg["sync"].close()
    sys.exit(0)

legs = {"exact": make_leg(None), "bucket": make_leg(True)}
# leg (a): four other batches take the four graphs (2 eager warm-ups + capture each)
others = [host_batch(1000 + s) for s in range(legs["exact"]["step"].max_graphs)]
for hb in others:
    for _ in range(legs["exact"]["step"].warm_steps + 1):
        legs["exact"]["step"](fresh(hb))
torch.cuda.synchronize()
assert legs["exact"]["step"].captures == legs["exact"]["step"].max_graphs, (legs["exact"]["step"].captures, legs["exact"]["step"].last_error)
del others
# both legs: once through the eight batches untimed (leg (b): warm-ups, capture, first replays)
for leg in legs.values():
    run_steps(leg, 2 * len(pool))
torch.cuda.synchronize()

rows = {k: [] for k in legs}
for rep in range(args.repeats):
    for name, leg in legs.items():
        st = leg["step"]
        before = (st.captures, st.replays, st.eager_steps)
        run_steps(leg, 4)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = run_steps(leg, args.steps)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.steps
        host = []
        for _ in range(3):
            b = fresh(pool[leg["n"] % len(pool)])
            leg["n"] += 1
            torch.cuda.synchronize()
            h0 = time.perf_counter()
            st(b)
            host.append((time.perf_counter() - h0) * 1e3)
        torch.cuda.synchronize()
        st.check()
        rows[name].append(dict(ms_per_step=round(ms, 3), host_queue_ms=round(sorted(host)[1], 3), loss=round(float(loss), 4),
                               captures=st.captures - before[0], replays=st.replays - before[1], eager_steps=st.eager_steps - before[2]))
        print(name, rep, rows[name][-1], flush=True)
hip.check_device_errors(dev)


def summary(name):
    r, st = rows[name], legs[name]["step"]
    ms = [x["ms_per_step"] for x in r]
    hq = [x["host_queue_ms"] for x in r]
    return dict(ms_per_step_mean=round(sum(ms) / len(ms), 3), ms_per_step_min=min(ms), ms_per_step_max=max(ms), spread_ms=round(max(ms) - min(ms), 3),
                host_queue_ms_median=sorted(hq)[len(hq) // 2], captures_total=st.captures, replays_total=st.replays, eager_steps_total=st.eager_steps,
                signatures=st.signatures, capture_error=st.last_error, repeats=r)


out = dict(tool="tools/varlen_graph_bench.py", device=torch.cuda.get_device_name(0), batch=args.batch, dims=dims, steps_per_repeat=args.steps,
           repeats=args.repeats, counts_rows_a_rows_b_scored_a_scored_b=counts, bucket_quanta=train.bucket_quanta(True),
           bounds=[list(b) for v in legs["bucket"]["step"]._known.values() for b in v],
           exact=summary("exact"), bucket=summary("bucket"))
a, b = out["exact"], out["bucket"]
out["bucket_minus_exact_ms"] = round(b["ms_per_step_mean"] - a["ms_per_step_mean"], 3)
out["within_spread_of_exact"] = bool(b["ms_per_step_mean"] - a["ms_per_step_mean"] <= a["spread_ms"])
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps({k: v for k, v in out.items() if k not in ("exact", "bucket")}), flush=True)
print("exact ", {k: v for k, v in a.items() if k != "repeats"})
print("bucket", {k: v for k, v in b.items() if k != "repeats"})
for leg in legs.values():
    leg["sync"].close()
hip.dropout_salt(dev).zero_()
