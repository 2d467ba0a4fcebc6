"""Two data-parallel ranks sharing the one GPU of the test box (gloo transport, the same hook /
bucket-view code path the RCCL run uses): the HIP training step with overlapped gradient exchange
keeps the replicas bit-identical and matches a single-process step on the concatenated batch's
averaged gradients."""
import os

import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, q, sparse):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mvp_pytorch_amd import dp, modeling, train
    from mvp_pytorch_amd.synthetic import synthetic_batch
    dev = torch.device("cuda:0")
    cfg = dict(gu.TINY_CFG, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    torch.manual_seed(0)
    model = modeling.BiBertImgForPreTraining(modeling.make_config(cfg)).to(dev)
    model.train()
    opt, sched = train.build_optimizer(model, lr=1e-3, t_total=10)
    if sparse:      # "default": what GradSync picks for the two-stage model (bf16 wire + row-sparse word table, dp.default_exchange)
        sync = dp.GradSync(model, bucket_mb=0.25)
        assert sync.comm_dtype == torch.bfloat16 and len(sync.sparse) == 1
    else:           # the conservative exchange: f32 wire, dense word table
        sync = dp.GradSync(model, bucket_mb=0.25, comm_dtype=torch.float32, sparse_rows=[])
    dims = dict(B=4, T=12, P=3, G=6, R=5)
    losses = []
    for step in range(3):
        batch = synthetic_batch(dims, cfg, 100 + 10 * step + rank, device=dev)
        torch.manual_seed(step)  # same hard-negative permutation draw on both ranks
        out = train.pretrain_step(model, batch, opt, sched, max_tag_length=dims["G"], grad_sync=sync, return_losses=True)
        losses.append(float(out[0]))
    torch.cuda.synchronize()
    probe = {n: p.detach().float().cpu().numpy() for n, p in model.named_parameters()
             if n in ("bert.txt_encoder.layer.0.attention.self.query.weight", "bert.embeddings.word_embeddings.weight",
                      "cls.predictions.decoder.weight", "logit_scale", "qa_head.weight")}
    n_sparse = sum(1 for b in sync.buckets if b["rows_of"] is not None)
    q.put((rank, losses, probe, len(sync.buckets), n_sparse))
    dist.destroy_process_group()


def _run(sparse):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = gu.free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, sparse)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(2)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return res


def test_two_rank_training_step_keeps_replicas_identical(dev):
    """The conservative exchange (f32 wire, dense), then GradSync's DEFAULT for the two-stage model (bf16 wire + the
    row-sparse exchange of the word-embedding gradient, GradSync.note_rows from train.pretrain_step): replicas identical in
    both, and both modes give the same parameters to the wire's rounding."""
    import numpy as np
    probes = []
    for sparse in (False, True):
        (_, l0, p0, nb, ns), (_, l1, p1, _, _) = _run(sparse)
        assert nb > 1 and ns == (1 if sparse else 0)
        assert all(np.isfinite(l0)) and all(np.isfinite(l1))
        for k in p0:
            assert np.array_equal(p0[k], p1[k]), k   # same averaged gradients -> identical replicas
        print("two-rank losses", "sparse" if sparse else "dense", l0, l1)
        probes.append((l0, p0))
    # two separate runs: equal up to the run-to-run reproducibility of atomically accumulated gradients (replicas INSIDE a
    # run are bit-identical, above); Adam moves an element by ~lr * sign(g), so noise-level gradients may flip single elements
    (ld, pd_), (ls, ps) = probes
    assert np.allclose(ld, ls, rtol=1e-3)
    for k in pd_:
        close = np.abs(pd_[k] - ps[k]) <= 2.5e-3
        assert close.mean() > 0.90, (k, float(close.mean()))     # rows outside the union are zero on both ranks; bf16 wire: 8 mantissa bits per summand


def test_bench_launcher_two_ranks_on_one_gpu(dev):
    """`python bench.py --gpus 2` as the driver starts it without a launcher: two rank processes, one JSON line from rank 0
    with n_gpus = 2 and the whole-job rate.  The test box has one GPU, so both ranks are pinned to it and talk through gloo
    (MVPTR_BENCH_DEVICE / MVPTR_DIST_BACKEND: the hooks bench.py has for exactly this); on a multi-GPU node the same code path
    runs one rank per GPU over RCCL."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MVPTR_BENCH_DEVICE="0", MVPTR_DIST_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    o = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "16",
                        "--full", "--no-extras"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert o.returncode == 0, o.stderr.decode()[-2000:]
    line = json.loads(o.stdout.decode().strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["steps"] == 2 and line["warmup"] == 1
    assert line["config"]["parallelism"] == "dp2" and line["config"]["global_batch"] == 32
    assert line["scaling"] == "weak" and line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - 32 / (line["ms_per_step"] * 1e-3)) < 0.02 * line["value"]
    # the N > 1 line checks what the ranks saw, times a second leg with the opt-ins and reports the
    # communication the step could not hide
    dpi = line["config"]["data_parallel"]
    assert dpi["rccl_ranks_seen"] == 2 and dpi["backend"] == "gloo" and dpi["rccl_version"] is None
    assert dpi["defaults"] == {"wire": "bf16", "sparse_word_table": True, "two_streams": False, "collective": "all_reduce"}
    assert dpi["dp_conservative"]["ms_per_step"] > 0 and dpi["dp_conservative"]["steps"] == 2 and dpi["dp_conservative"]["stalled_steps"] == 0
    assert "dp_rs_ag" not in dpi or "error" in dpi["dp_rs_ag"] or dpi["dp_rs_ag"]["ms_per_step"] > 0     # RCCL only
    assert isinstance(dpi["exposed_comm_ms"], float) and dpi["ms_per_step_without_exchange"] > 0
    # the ZeRO-1 leg (round 6): two ranks, each with the Adam moments of half of the chunk-padded arena
    zs = dpi["dp_sharded_optimizer"]
    assert "error" not in zs, zs
    assert zs["ms_per_step"] > 0 and zs["steps"] == 2 and zs["optimizer_state_elements_per_rank"] > 0
    assert line["config"]["max_grad_norm"] == 10.0


def test_bench_plain_run_is_lean_and_dumps_outputs(dev, tmp_path):
    """A plain `bench.py --gpus 1` times exactly --steps steps, runs no leg beside the headline (those need --full) and with
    --dump-outputs writes the loss and the weight sample of its last timed step."""
    import json
    import subprocess
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "MVPTR_BENCH_DEVICE"):
        env.pop(k, None)
    out = tmp_path / "dump"
    o = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "16",
                        "--dump-outputs", str(out)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert o.returncode == 0, o.stderr.decode()[-2000:]
    line = json.loads(o.stdout.decode().strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert abs(line["value"] - 16 / (line["ms_per_step"] * 1e-3)) < 0.02 * line["value"]
    cfg = line["config"]
    assert cfg["all_slots_valid"] is None and cfg["with_input_pipeline"] is None and cfg["host_enqueue_ms_per_step"] is None
    assert cfg["data_parallel"] is None and "secondary" not in cfg and "single_stream_model" not in cfg and "cpu_baseline" not in line
    assert "kernel" not in line["roofline"] and line["roofline"]["step_frac"] > 0
    hg = cfg["hip_graph"]
    if hg["captures"] == 1:       # 2 eager steps + the capture's own replay, then warm-up and timed steps: nothing else ran
        assert hg["eager_steps"] == 2 and hg["replayed_steps"] == 1 + 1 + 3, hg
    assert sorted(p.name for p in out.iterdir()) == ["loss.npy", "params_sample.npy"]
    loss, params = np.load(out / "loss.npy"), np.load(out / "params_sample.npy")
    assert loss.dtype == np.float32 and loss.shape == (1,) and abs(float(loss[0]) - cfg["final_loss"]) < 1e-3
    assert params.dtype == np.float32 and 1e6 < params.size < (64 << 20) // 4 and np.isfinite(params).all()


# ------------------------------------------------------------------------------ round-3: the RCCL path on one GPU
def _one_rank_worker(mode, port, q):
    """Three training steps of the tiny two-stage model in a fresh process.  mode:
    'plain'  no GradSync (gradients through autograd tensors)
    'arena'  GradSync without a process group (gradient arena only)
    'rccl' / 'rccl_opts'  init_process_group("nccl", world_size=1) + GradSync(force_collectives=True): hooks, bucket
             launches on RCCL's stream, ReduceOp.AVG, used-parameter bitmap, finish(); 'rccl_opts' adds the opt-ins
             (bf16 wire, row-sparse word table with its id all-gather + compact all-reduce, two compute streams)."""
    import time
    import torch.distributed as dist
    from mvp_pytorch_amd import dp, modeling, train
    from mvp_pytorch_amd.synthetic import synthetic_batch
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if mode.startswith("rccl"):
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    cfg = dict(gu.TINY_CFG, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    if mode == "rccl_opts":
        cfg["parallel_stacks"] = "always"
    torch.manual_seed(0)
    model = modeling.BiBertImgForPreTraining(modeling.make_config(cfg)).to(dev)
    model.train()
    opt, sched = train.build_optimizer(model, lr=1e-3, t_total=10)
    sync = None
    if mode == "arena":
        sync = dp.GradSync(model, bucket_mb=0.25)
    elif mode == "rccl":
        sync = dp.GradSync(model, bucket_mb=0.25, force_collectives=True, comm_dtype=torch.float32, sparse_rows=[])
    elif mode == "rccl_rsag":       # reduce-scatter + all-gather per bucket over its chunk-padded span
        sync = dp.GradSync(model, bucket_mb=0.25, force_collectives=True, comm_dtype=torch.float32, sparse_rows=[], collective="rs_ag")
    elif mode == "rccl_opts":
        sync = dp.GradSync(model, bucket_mb=0.25, force_collectives=True, comm_dtype=torch.bfloat16,
                           sparse_rows=[model.bert.embeddings.word_embeddings.weight])
    elif mode == "rccl_sharded":    # ZeRO-1: reduce-scatter, AdamW on the rank's shard of the flat parameter arena, all-gather of the parameters
        sync = dp.GradSync(model, bucket_mb=0.25, force_collectives=True, comm_dtype=torch.float32, shard_optimizer=True)
        opt, sched = train.build_optimizer(model, lr=1e-3, t_total=10, grad_sync=sync)
        from mvp_pytorch_amd.optimization import ShardedAdamW
        assert isinstance(opt, ShardedAdamW) and opt.moment_elements() == 2 * sync._arena.numel()
    dims = dict(B=4, T=12, P=3, G=6, R=5)
    names = ("bert.txt_encoder.layer.0.attention.self.query.weight", "bert.mul_encoder.layer.1.output.dense.bias",
             "bert.embeddings.word_embeddings.weight", "cls.predictions.decoder.weight", "bert.pooler.dense.weight",
             "bert.txt_proj", "logit_scale", "bert.img_embedding.weight", "half_mlm.transform.LayerNorm.weight")
    before = {n: p.detach().clone() for n, p in model.named_parameters() if n in names}
    losses, grads, info = [], {}, {}
    for step in range(3):
        batch = synthetic_batch(dims, cfg, 100 + 10 * step, device=dev)
        torch.manual_seed(step)
        # train.pretrain_step spelled out, to look at the exchange between its stages
        if sync is not None and sync.sparse:
            sync.note_rows(model.bert.embeddings.word_embeddings.weight, [batch["input_ids_a"], batch["input_ids_b"]])
        out = model(**train.model_inputs(batch, dims["G"]))
        out[0].backward()
        hooks = 0 if sync is None else sync._next          # buckets that went out from hooks, overlapped with backward
        if sync is not None:
            sync(want_norm=True)
            if sync.exchange:       # per-bucket partial sums behind the collectives = the pass over the whole arena, bit for bit
                n1 = sync.clip_coef(10.0)[0].clone()
                sync._norm_done = set()
                assert torch.equal(n1, sync.clip_coef(10.0)[0])
        if step == 0:   # gradients of the FIRST step: identical weights in every mode, only the exchange path differs
            grads = {n: p.grad.detach().float().cpu().numpy().copy() for n, p in model.named_parameters() if n in names and p.grad is not None}
        losses.append(float(out[0]))
        info = dict(buckets=0 if sync is None else len(sync.buckets), launched_from_hooks=hooks,
                    qa_none=model.qa_head.weight.grad is None, stalled=0 if sync is None else sync.stalled_steps)
        coef = train.clip_coefficient(model, sync, 10.0)
        if coef is not None:
            opt.step(grad_scale=coef)
        else:
            opt.step()
        sched.step()
        if sync is not None:
            sync.zero_grad()
        else:
            opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    delta = {n: (p.detach() - before[n]).float().cpu().numpy() for n, p in model.named_parameters() if n in names}
    q.put((mode, losses, delta, grads, info))
    if mode.startswith("rccl"):
        dist.destroy_process_group()


def _one_rank(mode):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = gu.free_port()
    p = ctx.Process(target=_one_rank_worker, args=(mode, port, q))
    p.start()
    res = q.get(timeout=600)
    p.join(timeout=120)
    assert p.exitcode == 0
    return res


def test_rccl_world1_and_gradient_arena_match_plain_step(dev):
    """the RCCL code path (backend nccl) run on the single GPU with a one-rank group, hooks forced on:
    same losses and, to the reproducibility of the atomically accumulated weight gradients, the same gradients and
    parameter updates as a step without any GradSync; the gradient arena alone (no process group) likewise."""
    import numpy as np
    ref = _one_rank("plain")
    for mode in ("arena", "rccl", "rccl_rsag", "rccl_opts", "rccl_sharded"):
        got = _one_rank(mode)
        print("one-rank", mode, got[1], got[4])
        assert np.allclose(got[1], ref[1], rtol=2e-4), (mode, got[1], ref[1])
        for n, gref in ref[3].items():      # first-step gradients: same weights everywhere, only the exchange path differs
            g = got[3][n]
            rel = np.linalg.norm(g - gref) / (np.linalg.norm(gref) + 1e-30)
            assert rel < (2e-2 if mode == "rccl_opts" else 2e-3), (mode, n, rel)    # bf16 wire: 8 mantissa bits
        for n, dref in ref[2].items():
            if n in ("logit_scale", "bert.txt_proj"):
                # contrastive branch: ill-conditioned (sums of cancelling terms), two Adam steps amplify run-to-run rounding
                assert np.isfinite(got[2][n]).all()
                continue
            d = got[2][n]
            # Adam moves an element by ~lr * sign(g): elements whose gradient is at the noise level may flip
            close = np.abs(d - dref) <= 2e-4 + 0.05 * np.abs(dref)
            assert close.mean() > (0.90 if mode == "rccl_opts" else 0.97), (mode, n, float(close.mean()))
        assert got[4]["qa_none"]                       # qa_head never used: grad None on the arena paths too (last step)
        if mode.startswith("rccl"):
            assert got[4]["buckets"] > 2 and got[4]["launched_from_hooks"] > 0    # overlapped launches happened
