"""Host-side logic on CPU: config / checkpoint surface, parameter tree vs the reference's
state_dict names, schedules (reference KAT), AdamW vs the oracle, synthetic batch invariants,
2-rank gloo gradient exchange, loud failure without a device."""
import json
import os
import tempfile

import numpy as np
import pytest
import torch

import golden_util as gu
from oracle import mvptr_oracle as orc


def _tiny_model(cls="BiBertImgForPreTraining", **over):
    from mvp_pytorch_amd import modeling
    cfg = dict(gu.TINY_CFG, **over)
    return getattr(modeling, cls)(modeling.make_config(cfg)), cfg


def test_param_tree_matches_reference_names():
    """gnorm:* keys of the fixtures are the reference's own named_parameters()."""
    d = gu.load("tiny_bi_pretrain")
    model, _ = _tiny_model()
    ours = dict(model.named_parameters())
    ref_names = [k[6:] for k in d if k.startswith("gnorm:")]
    assert len(ref_names) > 100
    for n in ref_names:
        assert n in ours, n
    # parameters the reference leaves without gradient in this step: only qa_head
    no_grad = sorted(set(ours) - set(ref_names))
    assert no_grad == ["qa_head.bias", "qa_head.weight"], no_grad
    d2 = gu.load("tiny_finetune")
    for prefix, cls, extra in (("ret_", "BiImageBertForRetrieval", dict(loss_type="ce")),
                               ("vqa_", "BiImageBertForVQA", dict(loss_type="bce", num_labels=37)),
                               ("ve_", "BiImageBertForSequenceClassification", dict(loss_type="ce", num_labels=3, classifier="linear"))):
        m, _ = _tiny_model(cls, **extra)
        ours = dict(m.named_parameters())
        for k in d2:
            if k.startswith(prefix + "gnorm:"):
                assert k[len(prefix) + 6:] in ours, k


def test_config_roundtrip_and_save_load():
    from mvp_pytorch_amd import modeling
    model, cfg = _tiny_model()
    with tempfile.TemporaryDirectory() as td:
        model.save_pretrained(td)
        assert sorted(os.listdir(td)) == ["config.json", "pytorch_model.bin"]
        c2 = modeling.BertConfig.from_pretrained(td, num_labels=5)
        assert c2.num_labels == 5 and c2.img_feature_dim == 2054 and c2.only_word_size == 1000
        m2 = modeling.BiBertImgForPreTraining.from_pretrained(td, config=modeling.BertConfig.from_pretrained(td))
        assert not m2.training  # from_pretrained leaves the model in eval mode
        for (n1, p1), (n2, p2) in zip(model.state_dict().items(), m2.state_dict().items()):
            assert n1 == n2
            if n1.endswith("decoder.weight"):
                continue  # re-cloned from the embeddings by tie_weights() (reference behaviour)
            assert torch.equal(p1, p2), n1
        emb = m2.bert.embeddings.word_embeddings.weight[:1000]
        assert torch.equal(m2.cls.predictions.decoder.weight, emb)
        assert torch.equal(m2.half_mlm.decoder.weight, emb)
        # legacy gamma/beta names and missing 'bert.' prefix are accepted
        sd = {k.replace("LayerNorm.weight", "LayerNorm.gamma").replace("LayerNorm.bias", "LayerNorm.beta"): v
              for k, v in model.state_dict().items()}
        m3 = modeling.BiBertImgForPreTraining.from_pretrained(td, config=c2, state_dict=sd)
        assert torch.equal(m3.bert.embeddings.LayerNorm.weight, model.bert.embeddings.LayerNorm.weight)
        # backbone-only checkpoint into a task model
        bsd = model.bert.state_dict()
        m4 = modeling.BiImageBertForRetrieval.from_pretrained(td, config=modeling.make_config(dict(cfg, loss_type="ce")), state_dict=bsd)
        assert torch.equal(m4.bert.txt_proj, model.bert.txt_proj)


def test_single_stream_ties_decoder():
    model, _ = _tiny_model("BertImgForPreTraining")
    assert model.cls.predictions.decoder.weight is model.bert.embeddings.word_embeddings.weight


def test_unsupported_options_raise():
    from mvp_pytorch_amd import modeling
    with pytest.raises(NotImplementedError):
        _tiny_model(hidden_act="relu")
    with pytest.raises(NotImplementedError):
        _tiny_model(img_feature_type="dis_code")
    with pytest.raises(ValueError):
        modeling.BertConfig(vocab_size_or_config_json_file=1.5)
    with pytest.raises(ValueError):
        modeling.BiBertImgModel({"not": "a config"})


def test_fails_loudly_without_device():
    model, _ = _tiny_model(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    d = gu.load("tiny_bi_pretrain")
    t = lambda k: torch.from_numpy(d["in:" + k])  # noqa: E731
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.bert.forward_single(input_ids_a=t("input_ids_a"), input_ids_b=t("input_ids_b"), img_feats=t("img_feats"),
                                  attention_mask_a=t("input_mask_a"), attention_mask_b=t("input_mask_b"))


def test_warmup_linear_schedule_kat():
    """transformers/pytorch_transformers/tests/optimization_test.py:105-110."""
    from mvp_pytorch_amd.optimization import AdamW, WarmupConstantSchedule, WarmupLinearSchedule
    p = torch.nn.Parameter(torch.zeros(1))
    opt = AdamW([p], lr=10.0)
    sch = WarmupLinearSchedule(opt, warmup_steps=2, t_total=10)
    lrs = []
    for _ in range(10):
        sch.step()
        lrs.append(opt.param_groups[0]["lr"])
    np.testing.assert_allclose(lrs, [5.0, 10.0, 8.75, 7.5, 6.25, 5.0, 3.75, 2.5, 1.25, 0.0], atol=1e-9)
    opt = AdamW([p], lr=10.0)
    sch = WarmupConstantSchedule(opt, warmup_steps=4)
    lrs = []
    for _ in range(10):
        sch.step()
        lrs.append(opt.param_groups[0]["lr"])
    np.testing.assert_allclose(lrs, [2.5, 5.0, 7.5, 10.0, 10.0, 10.0, 10.0, 10.0, 10.0, 10.0], atol=1e-9)


def test_adamw_matches_reference_step_and_converges():
    from mvp_pytorch_amd.optimization import AdamW
    d = gu.load("tiny_bi_pretrain")
    names = gu.ADAMW_PROBES
    from mvp_pytorch_amd.modeling import param_shapes
    shapes = param_shapes("BiBertImgForPreTraining", d["config"])
    det = gu.det_state_dict({n: shapes[n] for n in names}, int(d["seed"]))
    params = {n: torch.nn.Parameter(torch.from_numpy(det[n].copy())) for n in names if ("grad:" + n) in d}
    assert len(params) >= 3
    no_decay = ["bias", "LayerNorm.weight"]
    groups = [{"params": [p for n, p in params.items() if not any(x in n for x in no_decay)], "weight_decay": 0.01},
              {"params": [p for n, p in params.items() if any(x in n for x in no_decay)], "weight_decay": 0.0}]
    for n, p in params.items():
        p.grad = torch.from_numpy(d["grad:" + n].copy())
    AdamW(groups, lr=5e-3, eps=1e-8).step()
    for n, p in params.items():
        np.testing.assert_allclose(p.detach().numpy(), d["adamw:" + n], rtol=1e-5, atol=1e-7, err_msg=n)
    # optimization_test.py:58-70 — converges on a 3-element quadratic
    w = torch.nn.Parameter(torch.tensor([0.1, -0.2, -0.1]))
    target = torch.tensor([0.4, 0.2, -0.5])
    opt = AdamW([w], lr=2e-1, weight_decay=0.0)
    for _ in range(100):
        loss = torch.nn.functional.mse_loss(w, target)
        loss.backward()
        opt.step()
        w.grad.detach_()
        w.grad.zero_()
    np.testing.assert_allclose(w.detach().numpy(), target.numpy(), atol=1e-2)


def test_synthetic_batch_invariants():
    from mvp_pytorch_amd.synthetic import synthetic_batch
    cfg, dims = gu.BASE_CFG, dict(B=16, T=70, P=5, G=20, R=50)
    b = synthetic_batch(dims, cfg, 3)
    La = dims["T"] + dims["P"]
    assert b["img_feats"].shape == (16, 50, 2054) and b["input_ids_a"].shape == (16, La)
    assert b["input_mask_b"].shape == (16, 70) and b["lm_label_ids_b"].shape == (16, 70)
    for i in range(16):
        ma = b["input_mask_a"][i]
        n = int(ma.sum())
        assert torch.all(ma[:n] == 1) and torch.all(ma[n:] == 0)  # prefix-contiguous
        assert b["input_ids_a"][i, 0] == 101 and b["input_ids_a"][i, n - 1] == 102
        p0, p1 = b["phrase_index"][i].tolist()
        assert torch.all(b["input_ids_a"][i, p0:p1] >= cfg["only_word_size"])
        assert torch.all(b["lm_label_ids_a"][i, p0:p1] == -1)
        i0, i1 = b["image_index"][i].tolist()
        assert i0 == La and i1 - i0 >= 3
        assert int(b["input_mask_b"][i, 20:].sum()) == i1 - i0
        assert torch.all(b["img_feats"][i, i1 - i0:] == 0)
        assert (b["lm_label_ids_a"][i] > -1).any() and (b["lm_label_ids_b"][i] > -1).any()
        assert torch.all(b["lm_label_ids_b"][i, 20:] == -1)
    assert torch.all(b["segment_ids_a"] == 0) and torch.all(b["segment_ids_b"] == 1)
    f = synthetic_batch(dims, cfg, 3, fixed_length=True)
    assert int(f["input_mask_a"].sum()) == 16 * La and int(f["input_mask_b"].sum()) == 16 * 70


def _dp_worker(rank, world, port, q, comm_dtype=torch.float32):
    import torch.distributed as dist
    from mvp_pytorch_amd import dp
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Tanh(), torch.nn.Linear(16, 4), torch.nn.Linear(4, 2))
    unused = torch.nn.Linear(3, 3)  # never touched by the loss (like qa_head, modeling_vlbert.py:1184)
    m.add_module("unused", unused)
    # a head that every rank uses at first and that rank 1 skips in the last step (a shard without
    # masked tag rows skips half_mlm): launch ORDER must stay identical on both ranks
    sometimes = torch.nn.Linear(2, 2)
    m.add_module("sometimes", sometimes)
    # a head that produces its FIRST gradient in a later step, and on one rank only at first (qa_head
    # when qa_ans appears in later batches, modeling_vlbert.py:1264-1268): the other parameters'
    # buckets have been launched from hooks by then
    late = torch.nn.Linear(2, 3)
    m.add_module("late", late)
    sync = dp.GradSync(m, bucket_mb=0.0002, comm_dtype=comm_dtype)  # tiny buckets -> several collectives, launched from hooks
    assert len(sync.buckets) > 2
    results = []
    used = [p for n, p in m.named_parameters() if not n.startswith("unused")]

    def loss_fn(x, with_head, with_late):
        out = m[3](m[2](m[1](m[0](x))))
        # the same sub-module used twice in one graph (mul_encoder runs on the joint and the hard batch)
        loss = (out ** 2).sum() + m[3](m[2](torch.tanh(m[0](x * 0.5)))).sum()
        if with_head:
            loss = loss + sometimes(out).pow(2).sum()
        if with_late:
            loss = loss + late(out).pow(2).sum()
        return loss

    early = []
    for step in range(5):
        g = torch.Generator().manual_seed(100 * step + rank)
        x = torch.randn(5, 8, generator=g)
        with_head = not (step == 3 and rank == 1)
        with_late = (step == 2 and rank == 0) or step >= 3
        if step == 4:   # gradient accumulation: half the loss twice, the first backward without exchange
            with sync.no_sync():
                (0.5 * loss_fn(x, with_head, with_late)).backward()
            (0.5 * loss_fn(x, with_head, with_late)).backward()
        else:
            loss_fn(x, with_head, with_late).backward()
        early.append(sync._next)   # buckets launched from hooks, before finish()
        # the global-norm clip survives the overlap: with want_norm the partial sums of squares of every bucket are taken
        # right behind its collective; the coefficient from them equals the one from a pass over the whole arena BIT FOR BIT
        # (same chunk slots, same order), and both equal the norm of the averaged gradients
        sync(want_norm=(step % 2 == 0))
        assert (len(sync._norm_done) == len(sync.buckets)) == (step % 2 == 0)
        n1, c1 = [t.clone() for t in sync.clip_coef(0.05)]
        sync._norm_done = set()
        n2, c2 = [t.clone() for t in sync.clip_coef(0.05)]
        assert torch.equal(n1, n2) and torch.equal(c1, c2), (step, n1, n2)
        want = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters() if p.grad is not None))
        assert abs(float(n1) - float(want)) <= 1e-5 * max(1.0, float(want)), (step, float(n1), float(want))
        assert abs(float(c1) - min(1.0, 0.05 / (float(want) + 1e-6))) < 1e-5
        results.append([None if p.grad is None else p.grad.detach().clone().numpy() for p in m.parameters()])
        # reference: gradient of the same loss computed locally, to be averaged by the parent
        ref = torch.autograd.grad(loss_fn(x, with_head, with_late), used, allow_unused=True)
        results[-1].append([np.zeros(tuple(p.shape), dtype=np.float32) if r is None else r.numpy() for r, p in zip(ref, used)])
        sync.zero_grad()
    assert early[0] == 0 and early[1] > 0, early   # step 0 learns the hot set, then launches overlap backward
    # a second backward outside no_sync() after buckets went out must fail loudly, not corrupt them
    x = torch.randn(5, 8)
    loss_fn(x, True, True).backward()
    try:
        loss_fn(x, True, True).backward()
        raised = False
    except RuntimeError as e:
        raised = "no_sync" in str(e)
    assert raised
    sync()
    sync.zero_grad()
    vals = dp.all_reduce_metrics([float(rank + 1), 2.0, 3.0], torch.device("cpu"))
    q.put((rank, results, vals))
    dist.destroy_process_group()


@pytest.mark.parametrize("comm_dtype", [torch.float32, torch.bfloat16])
def test_grad_sync_two_ranks_gloo(comm_dtype):
    """world_size-2 gloo run of the overlapped bucketed all-reduce: hooks launch buckets during
    backward, gradients are averaged in place, unused parameters do not stall or desynchronise, a
    parameter whose first gradient arrives late is still exchanged, accumulation under no_sync()."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = gu.free_port()
    tol = 1e-5 if comm_dtype == torch.float32 else 2e-2
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, comm_dtype)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(2)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, r0, v0), (_, r1, v1) = res
    names = [n for n, _ in torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Tanh(), torch.nn.Linear(16, 4), torch.nn.Linear(4, 2),
                                              ).named_parameters()] + ["unused.weight", "unused.bias", "sometimes.weight", "sometimes.bias",
                                                                       "late.weight", "late.bias"]
    used_idx = [i for i, n in enumerate(names) if not n.startswith("unused")]
    for step in range(5):
        g0, g1 = r0[step], r1[step]
        local0, local1 = g0[-1], g1[-1]
        for j, i in enumerate(used_idx):
            want = (local0[j] + local1[j]) / 2
            if names[i].startswith("late") and step < 2:
                assert g0[i] is None and g1[i] is None, (step, names[i])   # nobody used it yet
                continue
            # a head one rank's shard skipped still gets the averaged gradient on BOTH ranks (the
            # skipping rank contributes zeros), so the replicas apply identical updates
            assert g0[i] is not None and g1[i] is not None, (step, names[i])
            scale = max(1.0, float(np.abs(want).max()))
            assert np.allclose(g0[i], want, atol=tol * scale), (step, names[i])
            assert np.array_equal(g0[i], g1[i]), (step, names[i])   # replicas hold identical gradients
        # unused params: no gradient (None, as under DDP find_unused_parameters) or zeros
        for i, n in enumerate(names):
            if n.startswith("unused"):
                assert g0[i] is None or np.all(g0[i] == 0)
                assert g1[i] is None or np.all(g1[i] == 0)
    assert v0 == v1 == [3.0, 4.0, 6.0]


def _dp_rs_ag_worker(rank, world, port, q):
    import torch.distributed as dist
    from mvp_pytorch_amd import dp
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(8, 300), torch.nn.Tanh(), torch.nn.Linear(300, 70), torch.nn.Linear(70, 2))
    sync = dp.GradSync(m, bucket_mb=0.01, comm_dtype=torch.float32, sparse_rows=[], collective="rs_ag")
    assert len(sync.buckets) > 2 and all(b["padded"] % world == 0 and b["padded"] % dp.NORM_CHUNK == 0 for b in sync.buckets)
    out = []
    for step in range(3):
        g = torch.Generator().manual_seed(10 * step + rank)
        x = torch.randn(6, 8, generator=g)
        (m(x) ** 2).sum().backward()
        sync(want_norm=True)
        norm, _ = sync.clip_coef(1.0)
        want = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters()))
        assert abs(float(norm) - float(want)) <= 1e-5 * max(1.0, float(want))
        ref = torch.autograd.grad((m(x) ** 2).sum(), list(m.parameters()))
        out.append(([p.grad.detach().clone().numpy() for p in m.parameters()], [r.numpy() for r in ref]))
        sync.zero_grad()
    q.put((rank, out))
    dist.destroy_process_group()


def test_rs_ag_layout_on_three_ranks_gloo():
    """collective='rs_ag' at a world size that is not a power of two (it used to refuse them): every bucket's span is
    padded to NORM_CHUNK x world elements, so the reduce-scatter shards divide evenly; on gloo the span goes out as one all-reduce
    (no reduce_scatter_tensor there), which checks the layout, the averaging and the per-bucket norm partial sums on 3 ranks."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = gu.free_port()
    procs = [ctx.Process(target=_dp_rs_ag_worker, args=(r, 3, port, q)) for r in range(3)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(3)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for step in range(3):
        for i in range(len(res[0][1][step][0])):
            want = sum(res[r][1][step][1][i] for r in range(3)) / 3
            for r in range(3):
                assert np.allclose(res[r][1][step][0][i], want, atol=1e-5 * max(1.0, float(np.abs(want).max())))
                assert np.array_equal(res[r][1][step][0][i], res[0][1][step][0][i])


def _dp_sparse_worker(rank, world, port, q, comm_dtype, early=False):
    import torch.distributed as dist
    from mvp_pytorch_amd import dp
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    emb = torch.nn.Embedding(400, 8)      # the "word table": only the looked-up rows get a gradient
    head = torch.nn.Linear(8, 3)
    m = torch.nn.ModuleDict(dict(emb=emb, head=head))
    sync = dp.GradSync(m, bucket_mb=0.0001, comm_dtype=comm_dtype, sparse_rows=[emb.weight])
    assert sum(1 for b in sync.buckets if b["rows_of"] is not None) == 1
    out = []
    for step in range(4):
        g = torch.Generator().manual_seed(10 * step + rank)
        ids_a = torch.randint(0, 400, (6, 5), generator=g)
        ids_b = torch.randint(0, 60, (6, 3), generator=g)
        # the ids are known before the step: note them BEFORE backward (a hot bucket is launched from
        # the gradient hook as soon as the table's gradient has landed)
        if early and step != 1:
            # round 6: the union formed host to host BEFORE the step (exchange_rows_early); the launch must not gather anything
            sync.exchange_rows_early(emb.weight, [torch.arange(400)] if step == 2 else [ids_a, ids_b, None])
            gathers = []
            real_all_gather = dist.all_gather
            dist.all_gather = lambda *a, **k: gathers.append(1) or real_all_gather(*a, **k)
        elif step == 1 and rank == 1:
            pass                          # a rank that notes nothing: every rank falls back to the dense exchange
        elif step == 2:
            sync.note_rows(emb.weight, [torch.arange(400)])   # union > half the table: dense is chosen
        elif not (early and step == 1):
            sync.note_rows(emb.weight, ids_a)
            sync.note_rows(emb.weight, [ids_b, None])
        used_union = None
        local = None
        orig = sync._row_union

        def spy(b):
            nonlocal used_union, local
            local = emb.weight.grad.detach().clone()   # this rank's own gradient, just before the exchange
            used_union = orig(b)
            return used_union

        sync._row_union = spy
        loss = head(emb(ids_a)).pow(2).sum() + head(emb(ids_b)).sum()
        loss.backward()
        sync()
        sync._row_union = orig
        if early and step != 1:
            dist.all_gather = real_all_gather
            assert not gathers and not sync._early_union      # nothing gathered inside the launch; the union was consumed
        out.append((local.numpy(), emb.weight.grad.detach().clone().numpy(), head.weight.grad.detach().clone().numpy(),
                    None if used_union is None else used_union.numpy()))
        sync.zero_grad()
    q.put((rank, out))
    dist.destroy_process_group()


@pytest.mark.parametrize("comm_dtype,early", [(torch.float32, False), (torch.bfloat16, False), (torch.float32, True)])
def test_grad_sync_row_sparse_gloo(comm_dtype, early):
    """Row-sparse exchange of an embedding-table gradient (world_size 2, gloo): only the union of the
    looked-up rows travels, the result equals the dense average; a rank without noted ids and a union
    larger than half the table both fall back to the dense all-reduce on every rank.  early: the union is formed ahead of the
    backward pass from HOST ids (exchange_rows_early, round 6) — same unions, same gradients, no all-gather inside the launch;
    a step without it (step 1: nothing noted either) takes the late form's dense fallback."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = gu.free_port()
    tol = 1e-6 if comm_dtype == torch.float32 else 2e-2
    procs = [ctx.Process(target=_dp_sparse_worker, args=(r, 2, port, q, comm_dtype, early)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(2)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, r0), (_, r1) = res
    for step in range(4):
        (l0, g0, h0, u0), (l1, g1, h1, u1) = r0[step], r1[step]
        want = (l0 + l1) / 2
        scale = max(1.0, float(np.abs(want).max()))
        assert np.allclose(g0, want, atol=tol * scale), step
        assert np.array_equal(g0, g1) and np.array_equal(h0, h1), step
        if step in (1, 2):
            assert u0 is None and u1 is None, step          # dense fallback on both ranks
        else:
            assert u0 is not None and np.array_equal(u0, u1), step
            touched = np.nonzero(np.abs(l0).sum(1) + np.abs(l1).sum(1))[0]
            assert set(touched) <= set(u0.tolist()) and len(u0) < 200


def test_flops_formula_matches_survey():
    import bench
    fwd, fb = bench.flops_per_pair(dict(B=256, T=70, P=5, G=20, R=50), bench.BASE_CFG, 11, 3)
    assert abs(fwd / 1e9 - 35.16) < 0.15  # 35.16 GFLOP forward per pair
    assert fb == 3 * fwd


def test_bench_dump_outputs_layout():
    """bench.py --dump-outputs: float32 loss + a sample of the weights at positions that are the same in every run."""
    import bench
    model = torch.nn.Sequential(torch.nn.Linear(300, 200), torch.nn.LayerNorm(200))
    loss = torch.tensor(1.25)
    with tempfile.TemporaryDirectory() as td:
        bench.dump_outputs(td, model, loss)
        l1, p1 = np.load(os.path.join(td, "loss.npy")), np.load(os.path.join(td, "params_sample.npy"))
        bench.dump_outputs(td, model, loss)
        p2 = np.load(os.path.join(td, "params_sample.npy"))
        assert sorted(os.listdir(td)) == ["loss.npy", "params_sample.npy"]
    n = bench.DUMP_SAMPLE_PER_TENSOR
    assert l1.dtype == np.float32 and l1.tolist() == [1.25]
    assert p1.dtype == np.float32 and p1.shape == (n + 200 + 200 + 200,) and np.array_equal(p1, p2)
    w = model[0].weight.detach().reshape(-1)
    idx = torch.randint(0, w.numel(), (n,), generator=torch.Generator().manual_seed(0))
    assert np.array_equal(p1[:n], w[idx].numpy())                      # 60 000 elements: sampled
    assert np.array_equal(p1[n:n + 200], model[0].bias.detach().numpy())   # small tensors: whole


def test_weight_caches_are_per_device():
    """WeightCache / PackList hand out one object per device (nn.DataParallel replicas share the
    owning module's attributes by reference): first device -> the object itself, others -> children."""
    import torch
    from mvp_pytorch_amd import engine
    c = engine.WeightCache()
    keys = iter([0, 0, 1, 1, 2, 0])
    orig = engine._dev_key
    engine._dev_key = lambda device: next(keys)
    try:
        a0, a0b, a1, a1b, a2, a0c = (c.for_device(None) for _ in range(6))
    finally:
        engine._dev_key = orig
    assert a0 is c and a0b is c and a0c is c
    assert a1 is a1b and a1 is not c and a2 is not a1 and a2 is not c
    c._key, a1._key = "x", "y"
    c.invalidate()
    assert c._key is None and a1._key is None
    pl = engine.PackList(engine.LayerPack() for _ in range(3))
    keys = iter([3, 5, 5, 3])
    engine._dev_key = lambda device: next(keys)
    try:
        p3, p5, p5b, p3b = (pl.for_device(None) for _ in range(4))
    finally:
        engine._dev_key = orig
    assert p3 is pl and p3b is pl and p5 is p5b and p5 is not pl and len(p5) == 3 and p5.group is not pl.group
    assert engine._dev_key(torch.device("cpu")) == -1


def _dp_nosync_worker(rank, world, port, q):
    import torch.distributed as dist
    from mvp_pytorch_amd import dp
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    body = torch.nn.Linear(6, 4)
    head = torch.nn.Linear(4, 2)       # used ONLY inside no_sync() (qa_head when qa_ans is present in the earlier micro-batches only)
    idle = torch.nn.Linear(4, 3)       # used in step 0 only: goes hot, must be demoted again
    m = torch.nn.ModuleDict(dict(body=body, head=head, idle=idle))
    sync = dp.GradSync(m, bucket_mb=0.0001, demote_after=2)
    out = []
    for step in range(5):
        g = torch.Generator().manual_seed(7 * step + rank)
        x = torch.randn(3, 6, generator=g)
        with sync.no_sync():
            l1 = head(body(x)).pow(2).sum()
            if step == 0:
                l1 = l1 + idle(body(x)).sum()
            l1.backward()
        body(x * 0.5).sum().backward()
        sync()
        hot_idle = idle.weight in (sync._hot or set())
        out.append((None if head.weight.grad is None else head.weight.grad.clone().numpy(),
                    torch.autograd.grad(head(body(x)).pow(2).sum(), head.weight)[0].numpy(), hot_idle, sync.stalled_steps))
        sync.zero_grad()
    q.put((rank, out))
    dist.destroy_process_group()


def test_grad_sync_head_used_only_under_no_sync_gloo():
    """a parameter that only received gradients in the accumulation micro-batches (inside no_sync())
    must count as used — its accumulated gradient is exchanged in finish() and kept, not set to None.  Also: a
    parameter that stops producing gradients is demoted from the hot set after `demote_after` idle steps, so
    it no longer holds back the hook launches of later hot buckets."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = gu.free_port()
    procs = [ctx.Process(target=_dp_nosync_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(2)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, r0), (_, r1) = res
    for step in range(5):
        g0, l0, hot0, _ = r0[step]
        g1, l1, hot1, _ = r1[step]
        assert g0 is not None and g1 is not None, step
        assert np.allclose(g0, (l0 + l1) / 2, atol=1e-5) and np.array_equal(g0, g1), step
        assert hot0 == hot1
    assert r0[0][2] and r0[1][2] and not r0[3][2] and not r0[4][2]     # hot after step 0, demoted after two idle steps
    assert r0[4][3] >= 1       # `head` never becomes ready in the exchanging backward: those steps are counted as stalled


def test_grad_arena_single_process_direct_delivery():
    """World size 1, no process group: GradSync is the gradient arena.  Encoder-layer-like units are laid out back
    to back in the unit's order, an autograd function can accumulate into the arena (`arena` / `direct` /
    `delivered`) instead of returning gradients, parameters nobody touched end with grad = None (the optimizer
    skips them), a tied row-sparse parameter is rejected."""
    from mvp_pytorch_amd import dp, engine

    class Layer(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Parameter(torch.randn(3, 2))
            self.b = torch.nn.Parameter(torch.randn(2))
            self.c = torch.nn.Parameter(torch.randn(4))

        def grad_arena_units(self):
            return [[self.c, self.a, self.b]]       # kernel order differs from registration order

    class Direct(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, a, b, c):
            ctx.ps = (a, b, c)
            ctx.save_for_backward(x)
            return (x @ a + b).sum() + (c * 2).sum()

        @staticmethod
        def backward(ctx, g):
            (x,) = ctx.saved_tensors
            a, b, c = ctx.ps
            flat = engine.grad_sink().arena([c, a, b])
            assert flat is not None and flat.numel() == 4 + 6 + 2
            flat[:4] += 2 * g
            flat[4:10] += (x.sum(0)[:, None].expand(3, 2) * g).reshape(-1)
            flat[10:] += x.shape[0] * g
            for p in (a, b, c):
                engine.grad_sink().delivered(p)
            return None, None, None, None

    torch.manual_seed(0)
    layer = Layer()
    other = torch.nn.Linear(2, 2)
    unused = torch.nn.Linear(2, 2)
    m = torch.nn.ModuleDict(dict(layer=layer, other=other, unused=unused))
    sync = dp.GradSync(m)
    assert engine.grad_sink() is sync and not sync.exchange
    x = torch.randn(5, 3)
    (Direct.apply(x, layer.a, layer.b, layer.c) + other(torch.ones(1, 2)).sum()).backward()
    sync()
    assert torch.allclose(layer.c.grad, torch.full((4,), 2.0))
    assert torch.allclose(layer.a.grad, x.sum(0)[:, None].expand(3, 2)) and torch.allclose(layer.b.grad, torch.full((2,), 5.0))
    assert other.weight.grad is not None and unused.weight.grad is None and unused.bias.grad is None
    # the unit is contiguous in the arena, in unit order
    assert layer.a.grad.data_ptr() == layer.c.grad.data_ptr() + 16 and layer.b.grad.data_ptr() == layer.a.grad.data_ptr() + 24
    sync.zero_grad()
    assert unused.weight.grad is not None and float(layer.a.grad.abs().sum()) == 0.0
    # tied row-sparse parameter
    emb = torch.nn.Embedding(10, 4)
    dec = torch.nn.Linear(4, 10, bias=False)
    dec.weight = emb.weight
    tied = torch.nn.ModuleDict(dict(emb=emb, dec=dec))
    with pytest.raises(ValueError):
        dp.GradSync(tied, sparse_rows=[emb.weight])
    engine.set_grad_sink(None)


def _dp_direct_worker(port, q):
    """One gloo rank with force_collectives: a parameter used by TWO calls of a directly delivering function becomes
    ready (its bucket launches) only after the second delivery; arena values equal the autograd result."""
    import torch.distributed as dist
    from mvp_pytorch_amd import dp, engine
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=0, world_size=1)

    class Scale(torch.autograd.Function):          # y = x * w, gradient of w delivered into the arena
        @staticmethod
        def forward(ctx, x, w):
            ctx.save_for_backward(x)
            ctx.w = w
            engine.note_uses(ctx, (w,), 1)
            return x * w

        @staticmethod
        def backward(ctx, g):
            (x,) = ctx.saved_tensors
            buf, direct = engine.grad_buffer(ctx.w)
            buf += (g * x).sum(0)
            launched.append(sync._next)
            return g * ctx.w, engine.grad_result(ctx.w, buf, direct)

    torch.manual_seed(0)
    m = torch.nn.ParameterDict(dict(w=torch.nn.Parameter(torch.randn(4)), v=torch.nn.Parameter(torch.randn(4))))
    sync = dp.GradSync(m, bucket_mb=1e-6, force_collectives=True)
    launched = []
    res = []
    for step in range(3):
        launched.clear()
        x = torch.randn(3, 4)
        y = Scale.apply(Scale.apply(x, m["w"]), m["w"]) * m["v"]
        y.sum().backward()
        nxt = sync._next
        sync()
        ref = torch.autograd.grad((x * m["w"].detach().requires_grad_(False) * 1.0).sum(), [], allow_unused=True) if False else None
        w = m["w"].detach().clone().requires_grad_(True)
        ((x * w * w) * m["v"].detach()).sum().backward()
        res.append((m["w"].grad.clone().numpy(), w.grad.numpy(), list(launched), nxt, len(sync.buckets)))
        sync.zero_grad()
    q.put(res)
    dist.destroy_process_group()


def test_direct_delivery_counts_uses_before_launch():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_dp_direct_worker, args=(34500 + (os.getpid() % 2000), q))
    p.start()
    res = q.get(timeout=120)
    p.join(timeout=60)
    assert p.exitcode == 0
    for step, (g, ref, launched, nxt, nb) in enumerate(res):
        assert np.allclose(g, ref, rtol=1e-5), step
        assert nb == 2
        if step > 0:
            # hot from step 1 on: w's bucket (index 0; v's bucket 1 is ready first but waits for its predecessor) must not
            # have been launched when the second delivery of w starts (launched[k] = buckets launched at the time of
            # backward call k), and both are out once backward has finished
            assert launched == [0, 0] and nxt == 2, (step, launched, nxt)


def test_two_grad_syncs_in_one_process_and_mixed_use_is_detected():
    """VERDICT r03 #9 / ADVICE r03: the gradient arena is looked up per parameter, so two models with their own GradSync
    coexist; a parameter that receives a gradient through the engine (direct delivery) AND through a torch op in one
    graph is reported instead of silently losing the torch-side contribution's ordering."""
    import torch.distributed as dist
    from mvp_pytorch_amd import dp, engine
    assert not dist.is_initialized()
    m1, m2 = torch.nn.Linear(3, 2), torch.nn.Linear(3, 2)
    s1, s2 = dp.GradSync(m1), dp.GradSync(m2)
    assert engine.grad_sink(m1.weight) is s1 and engine.grad_sink(m2.weight) is s2 and engine.grad_sink(m2.bias) is s2
    g1, d1 = engine.grad_buffer(m1.weight)
    g2, d2 = engine.grad_buffer(m2.weight)
    assert d1 and d2 and g1.data_ptr() == m1.weight.grad.data_ptr() and g2.data_ptr() == m2.weight.grad.data_ptr()
    assert g1.data_ptr() != g2.data_ptr()
    foreign = torch.nn.Parameter(torch.zeros(2))
    assert engine.grad_sink(foreign) is None and not engine.grad_buffer(foreign)[1]
    engine.set_grad_sink(None)
    assert engine.grad_sink(m1.weight) is None

    # mixed use under an exchanging arena: simulated with the delivery protocol on a one-rank gloo group
    port = gu.free_port()
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        lin = torch.nn.Linear(2, 2)
        sync = dp.GradSync(lin, force_collectives=True, check_mixed_use=True)

        class Deliver(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, w):
                ctx.w = w
                engine.note_uses(ctx, (w,), 1)
                return x.sum() + 0 * w.sum()

            @staticmethod
            def backward(ctx, g):
                buf, direct = engine.grad_buffer(ctx.w)
                assert direct
                buf += 1.0
                return None, engine.grad_result(ctx.w, buf, direct)

        x = torch.ones(1, 2)
        # engine path + a plain torch use of the same parameter in one graph -> detected in the hook
        with pytest.raises(RuntimeError, match="one path per parameter"):
            (Deliver.apply(x, lin.weight) + (lin.weight * 2).sum() + lin.bias.sum()).backward()
        engine.set_grad_sink(None)
    finally:
        dist.destroy_process_group()


def test_adamw_single_tensor_path_takes_the_clip_coefficient():
    """a parameter whose step counter differs from its group's (a head that first receives a gradient at a
    later step) goes through AdamW._single, which must multiply the gradient by the clip coefficient like the fused paths."""
    from mvp_pytorch_amd.optimization import AdamW
    torch.manual_seed(3)

    def run(scaled):
        a = torch.nn.Parameter(torch.linspace(-1, 1, 6).reshape(2, 3).clone())
        b = torch.nn.Parameter(torch.linspace(0.5, 1.5, 4).clone())
        opt = AdamW([a, b], lr=1e-2, weight_decay=0.01)
        ga1, ga2, gb2 = torch.full((2, 3), 0.3), torch.full((2, 3), -0.7), torch.tensor([1.0, -2.0, 3.0, -4.0])
        a.grad = ga1.clone()                      # step 1: only `a` has a gradient
        opt.step()
        if scaled:                                # step 2: both, clip coefficient 0.25 through grad_scale
            a.grad, b.grad = ga2.clone(), gb2.clone()
            opt.step(grad_scale=torch.tensor([0.25]))
        else:                                     # the same with the gradients scaled beforehand
            a.grad, b.grad = ga2 * 0.25, gb2 * 0.25
            opt.step()
        return a.detach().clone(), b.detach().clone()

    a1, b1 = run(True)
    a2, b2 = run(False)
    assert torch.allclose(a1, a2, atol=1e-7) and torch.allclose(b1, b2, atol=1e-7)


def test_stream_policy_by_backend(monkeypatch):
    """Two compute streams: single rank yes; multi-rank over RCCL yes (same schedule at every N); over gloo no; "always" /
    "single_rank" / False override (modeling_vlbert._streams_allowed; callers AND it with bool(parallel_stacks))."""
    import torch.distributed as dist
    from mvp_pytorch_amd.modeling.modeling_vlbert import _streams_allowed
    assert _streams_allowed(True) and _streams_allowed("always") and _streams_allowed("single_rank")     # no process group
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 8)
    monkeypatch.setattr(dist, "get_backend", lambda *a, **k: "nccl")
    assert _streams_allowed(True) and _streams_allowed("always") and not _streams_allowed("single_rank")
    monkeypatch.setattr(dist, "get_backend", lambda *a, **k: "gloo")
    assert not _streams_allowed(True) and _streams_allowed("always") and not _streams_allowed("single_rank")
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 1)
    assert _streams_allowed(True) and _streams_allowed("single_rank")


def test_device_error_word_host_side():
    """hip.flag_device_error_if / engine.AsyncCounts on CPU tensors: the host can look at once, so the check raises in place
    (the device path — a word carried along with every count copy — is covered by tests/test_ops_gpu.py::test_compact_scored_rows)."""
    import torch
    from mvp_pytorch_amd import engine, hip
    hip.flag_device_error_if(torch.tensor(False), hip.DEV_ERR_PHRASES)
    with pytest.raises(RuntimeError, match="max_phrases"):
        hip.flag_device_error_if(torch.tensor(True), hip.DEV_ERR_PHRASES)
    assert engine.AsyncCounts([torch.tensor(3), torch.tensor(9)]).get() == [3, 9]
    with pytest.raises(RuntimeError, match="device-side check failed: .*3 valid regions"):
        hip.raise_device_error(hip.DEV_ERR_FEW_REGIONS)
    hip.raise_device_error(0)


def _sharded_worker(rank, world, port, q, comm_dtype):
    """two (or one) ranks: the same toy model trained 4 steps with the replicated optimizer (GradSync all-reduce + AdamW) and with the
    ZeRO-1 path (GradSync(shard_optimizer=True) + ShardedAdamW) — parameters must be bit-equal after every step"""
    import torch.distributed as dist
    from mvp_pytorch_amd import dp, train
    from mvp_pytorch_amd.optimization import AdamW, ShardedAdamW, WarmupLinearSchedule
    if world > 1:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)

    def build():
        torch.manual_seed(0)
        m = torch.nn.Sequential(torch.nn.Linear(24, 40), torch.nn.Tanh(), torch.nn.Linear(40, 24), torch.nn.LayerNorm(24), torch.nn.Linear(24, 3))
        m.add_module("unused", torch.nn.Linear(3, 3))       # never produces a gradient: skipped by both optimizers
        return m

    def groups(m):
        named = list(m.named_parameters())
        return [{"params": [p for n, p in named if "bias" not in n], "weight_decay": 0.01},
                {"params": [p for n, p in named if "bias" in n], "weight_decay": 0.0}]

    out = {}
    for mode in ("replicated", "sharded"):
        m = build()
        if mode == "sharded":
            sync = dp.GradSync(m, bucket_mb=0.002, comm_dtype=comm_dtype, shard_optimizer=True)
            opt = ShardedAdamW(groups(m), sync, lr=1e-2, eps=1e-8)
            assert all(p.data.data_ptr() >= sync._parena.data_ptr() for p in m.parameters())      # views into the flat parameter arena
        else:
            sync = dp.GradSync(m, bucket_mb=0.002, comm_dtype=comm_dtype, sparse_rows=[], force_collectives=world > 1)
            opt = AdamW(groups(m), lr=1e-2, eps=1e-8)
        sched = WarmupLinearSchedule(opt, warmup_steps=2, t_total=10)
        assert len(sync.buckets) >= 2
        snaps = []
        for step in range(4):
            g = torch.Generator().manual_seed(100 * step + rank)
            x = torch.randn(6, 24, generator=g)
            loss = (m[4](m[3](m[2](m[1](m[0](x))))) ** 2).sum()
            loss.backward()
            sync(want_norm=True)
            coef = sync.clip_coef(0.5)[1]        # (train.clip_coefficient takes this path on a HIP device; the arena math is the same on the CPU)
            opt.step(grad_scale=coef)
            sched.step()
            sync.zero_grad()
            snaps.append([p.detach().clone().numpy() for p in m.parameters()])
        out[mode] = snaps
        if mode == "sharded":
            out["moments"] = opt.moment_elements()
            out["arena"] = int(sync._arena.numel())
        sync.close()
    q.put((rank, out))
    if world > 1:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,comm_dtype", [(1, torch.float32), (2, torch.float32), (2, torch.bfloat16)])
def test_sharded_optimizer_equals_replicated(world, comm_dtype):
    """VERDICT r05 #7 (ZeRO-1 over the buckets): reduce-scatter (emulated on gloo: all-reduce, own slice) + per-shard clip partial sums +
    AdamW on the shard + all-gather of the updated PARAMETERS against the replicated path, bit for bit after each of four steps under a
    warm-up schedule and the global-norm clip, on both ranks; the rank holds the moments of 1 / world of the (chunk-padded) arena."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = gu.free_port()
    procs = [ctx.Process(target=_sharded_worker, args=(r, world, port, q, comm_dtype)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(world)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, out in res:
        for step in range(4):
            for a, b in zip(out["replicated"][step], out["sharded"][step]):
                assert np.array_equal(a, b), (rank, step, np.abs(a - b).max())
        assert out["moments"] == 2 * out["arena"] // world
    if world == 2:
        for a, b in zip(res[0][1]["sharded"][3], res[1][1]["sharded"][3]):
            assert np.array_equal(a, b)          # replicas stay identical
    first, last = res[0][1]["sharded"][0], res[0][1]["sharded"][3]
    assert any(not np.array_equal(a, b) for a, b in zip(first, last))       # and they did train
