"""GraphedStep(bucket=...): bounded uni-modal passes and one captured graph for variable-length batches (needs an MI355X)."""
import numpy as np
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu

DIMS = dict(B=16, T=12, P=3, G=6, R=5)
SEEDS = list(range(40, 48))


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _pin_randperm(request, dev):
    perm_dev = torch.randperm(DIMS["B"], generator=torch.Generator().manual_seed(9)).to(dev)
    orig = torch.randperm
    torch.randperm = lambda n, *a, **k: perm_dev
    request.addfinalizer(lambda: setattr(torch, "randperm", orig))


def _model_kwargs(batch, host_counts):
    return dict(input_ids_a=batch["input_ids_a"], token_type_ids_a=batch["segment_ids_a"], attention_mask_a=batch["input_mask_a"],
                masked_lm_labels_a=batch["lm_label_ids_a"], input_ids_b=batch["input_ids_b"], img_feats=batch["img_feats"],
                token_type_ids_b=batch["segment_ids_b"], attention_mask_b=batch["input_mask_b"], masked_lm_labels_b=batch["lm_label_ids_b"],
                max_tag_length=DIMS["G"], host_counts=host_counts)


# ------------------------------------------------------------------------------------------------------------------------
def test_bounded_pack_maps_stay_inside_the_bound(dev):
    """mvptr_pack_maps_bounded alone (no model step): with a limit at or above the count the maps equal the unbounded ones and the
    index vector reads -1 from the count to the limit; with a limit BELOW the count nothing the maps hold names a row at or past
    the limit — sequence extents end there, later slots read as padding — while the counts keep the true totals."""
    from mvp_pytorch_amd import hip
    from mvp_pytorch_amd.modeling.modeling_vlbert import additive_mask
    from mvp_pytorch_amd.synthetic import synthetic_batch
    b = synthetic_batch(DIMS, gu.TINY_CFG, 43, device=dev)
    B, La = b["input_mask_a"].shape
    mask = additive_mask(b["input_mask_a"])
    seg = [dict(mask=mask, len=La, src_seq_stride=La)]
    pos0, idx0, st0, ln0, cnt0 = hip.pack_maps(seg, B)
    rows = int(cnt0[0])
    assert rows == b["host_counts"]["rows_a"]
    for limit in (rows, rows + 13, B * La):
        pos, idx, st, ln, cnt = hip.pack_maps(seg, B, row_limit=limit)
        assert idx.numel() == limit
        assert torch.equal(pos, pos0) and torch.equal(st, st0) and torch.equal(ln, ln0) and torch.equal(cnt, cnt0)
        assert torch.equal(idx[:rows], idx0[:rows]) and bool((idx[rows:] == -1).all())
    limit = rows - 37
    pos, idx, st, ln, cnt = hip.pack_maps(seg, B, row_limit=limit)
    torch.cuda.synchronize()
    assert torch.equal(cnt, cnt0)                                      # the true totals: mvptr_check_bounds reports from them
    assert idx.numel() == limit and torch.equal(idx, idx0[:limit])
    assert int(pos.max()) == limit - 1 and int((st + ln).max()) == limit and int(st.min()) >= 0 and int(ln.min()) >= 0
    keep = pos0 < limit
    assert torch.equal(pos, torch.where(keep, pos0, torch.full_like(pos0, -1)))
    assert torch.equal(ln, (pos >= 0).sum(1).to(ln.dtype))
    # a second-stage map over the clamped positions: a slot its source map left without a row becomes a zero row (-1), not row
    # src_base - 1
    posj, idxj, stj, lnj, cntj = hip.pack_maps([dict(mask=mask, len=La, pos=pos, src_base=1000)], B, fill_idx=True)
    torch.cuda.synchronize()
    got = idxj[:rows]
    assert int((got == -1).sum()) == rows - limit and int(got[got >= 0].min()) == 1000 and int(got.max()) == 1000 + limit - 1


@pytest.mark.parametrize("how", ["tight", "full"])
@pytest.mark.parametrize("seed", [40, 43, 46])
def test_bounded_forward_backward_equals_exact(dev, seed, how, request):
    """The model called with bounds in host_counts (uni-modal passes on bound-sized buffers with the row count on the device,
    bound-many scored-row slots) against the model called with the exact host_counts: same losses (5e-4 relative) and gradients
    (1e-2 relative L2; attention.self.key.bias excluded, its true gradient is zero) — the tolerances
    test_sync_free_joint_pass_and_host_counts holds the bound-sized joint pass to.  bounds = the counts themselves (tight) and
    = every slot of the padded batch (full).  engine.AsyncCounts is never awaited inside a step."""
    from mvp_pytorch_amd import engine, hip, modeling
    from mvp_pytorch_amd.modeling.modeling_vlbert import BOUND_KEYS
    from mvp_pytorch_amd.synthetic import synthetic_batch
    from mvp_pytorch_amd.train import COUNT_KEYS, batch_caps, bucket_bounds
    cfg = dict(gu.TINY_CFG, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, max_phrases=3)
    batch = synthetic_batch(DIMS, cfg, seed, device=dev)
    _pin_randperm(request, dev)
    hc = batch["host_counts"]
    counts = tuple(int(hc[k]) for k in COUNT_KEYS)
    caps = batch_caps(batch)
    bounds = bucket_bounds(counts, caps, (1, 1)) if how == "tight" else caps
    assert bounds == (counts if how == "tight" else caps)
    res, waits = {}, {}
    orig_get = engine.AsyncCounts.get
    hip.check_device_errors(dev)
    for mode in ("exact", "bounded"):
        torch.manual_seed(0)
        model = modeling.BiBertImgForPreTraining(modeling.make_config(cfg)).to(dev)
        model.train()
        kw = _model_kwargs(batch, hc if mode == "exact" else type(hc)(hc, **dict(zip(BOUND_KEYS, bounds))))
        n_wait = [0]

        def counting_get(self, _n=n_wait):
            if not self.ready():
                _n[0] += 1
            return orig_get(self)

        engine.AsyncCounts.get = counting_get
        try:
            for _ in range(3):
                model.zero_grad(set_to_none=True)
                out = model(**kw)
                out[0].backward()
                torch.cuda.synchronize()
        finally:
            engine.AsyncCounts.get = orig_get
        waits[mode] = n_wait[0]
        res[mode] = ([float(x) for x in out], {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None})
    hip.check_device_errors(dev)
    print("seed", seed, how, "counts", counts, "bounds", bounds, "waits", waits)
    assert waits["bounded"] == 0
    la, lb = np.array(res["exact"][0]), np.array(res["bounded"][0])
    print("exact", la, "bounded", lb, "rel", np.abs(la - lb).max() / np.abs(la).max())
    ga, gb = res["exact"][1], res["bounded"][1]
    assert set(ga) == set(gb)
    worst = max((_rel(gb[n], ga[n]), n) for n in ga if ga[n].norm() > 1e-6 and not n.endswith("attention.self.key.bias"))
    print("worst gradient rel L2", worst)
    assert np.abs(la - lb).max() / np.abs(la).max() < 5e-4
    assert worst[0] < 1e-2, worst


# ------------------------------------------------------------------------------------------------------------------------
def _run_steps(dev, cfg, host_batches, steps, stepper_kw, keep_wra):
    """the model / optimizer / schedule of test_graphed_step_matches_eager_steps, stepped over `host_batches` cycled, every call
    with newly allocated device tensors (the previous ones dropped)"""
    from mvp_pytorch_amd import dp, engine, hip, modeling, train
    from mvp_pytorch_amd.optimization import AdamW, WarmupLinearSchedule
    torch.manual_seed(0)
    engine._seed_counter[0] = 0x5DEECE66D
    model = modeling.BiBertImgForPreTraining(modeling.make_config(cfg))
    sd = {k: torch.from_numpy(v) for k, v in gu.det_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 17, 1.0).items()}
    model.load_state_dict(sd)
    model.to(dev).train()
    opt = AdamW([{"params": list(model.parameters()), "weight_decay": 0.01}], lr=1e-3, eps=1e-8)
    sched = WarmupLinearSchedule(opt, warmup_steps=10, t_total=100)
    sync = dp.GradSync(model)
    stepper = train.GraphedStep(model, opt, sched, max_tag_length=DIMS["G"], max_grad_norm=1.0, grad_sync=sync, **stepper_kw)
    losses, kinds = [], []
    batch = None
    for i in range(steps):
        hb = host_batches[i % len(host_batches)]
        batch = None                                      # drop the previous device tensors before the new ones are allocated
        batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in hb.items() if keep_wra or k not in ("phrase_index", "image_index")}
        before = (stepper.replays, stepper.eager_steps, stepper.captures)
        losses.append(float(stepper(batch)))
        kinds.append((stepper.replays - before[0], stepper.eager_steps - before[1], stepper.captures - before[2]))
    stepper.check()
    torch.cuda.synchronize()
    hip.check_device_errors(dev)
    upd = {n: (p.detach().float().cpu() - sd[n].float()) for n, p in model.named_parameters()}
    steps_seen = {int(opt.state[p]["step"]) for p in model.parameters() if p in opt.state and len(opt.state[p])}
    sync.close()
    return losses, upd, steps_seen, stepper, kinds


def _upd_rel(x, y):
    num = sum(float((x[n] - y[n]).pow(2).sum()) for n in x)
    den = sum(float(y[n].pow(2).sum()) for n in x)
    return (num / den) ** 0.5


def _host_batches(cfg):
    from mvp_pytorch_amd.synthetic import synthetic_batch
    return [synthetic_batch(DIMS, cfg, s) for s in SEEDS]


@pytest.mark.parametrize("quanta,first", [((1024, 256), 40), ((32, 8), 40), ((32, 8), 41)])
def test_eight_different_batches_replay_one_graph(dev, quanta, first, request):
    """24 steps over eight batches with eight different sets of counts, each call on newly allocated device tensors: eager, eager
    again (the noise of the f32 atomics) and GraphedStep(bucket=...).  Quanta 1024 / 256: ONE signature, one capture, every step
    after the two warm-ups a replay.  Quanta 32 / 8: at most two captures and nothing but replays after the last one (in seed order
    the first batch's bounds cover all eight; started at seed 41 the smaller bounds come first and seed 43 needs a second set).  Numerical
    bounds of test_graphed_step_matches_eager_steps: per-step losses within 2e-5 + 4 x noise, total update within
    max(1e-2, 2 x noise) relative L2, optimizer step counters at 24.  A stale input cannot pass: the losses of a cycle differ
    from batch to batch and every replayed loss sits on the eager loss of ITS batch."""
    from mvp_pytorch_amd import hip
    cfg = dict(gu.TINY_CFG, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, max_phrases=3)
    hbs = _host_batches(cfg)
    hbs = hbs[first - SEEDS[0]:] + hbs[:first - SEEDS[0]]
    assert len({tuple(sorted(dict(b["host_counts"]).items())) for b in hbs}) == 8      # eight exact signatures
    _pin_randperm(request, dev)
    steps, warm = 24, 2
    salt0 = int(hip.dropout_salt(dev).item())
    l_a, u_a, s_a, _, _ = _run_steps(dev, cfg, hbs, steps, dict(enabled=False), False)
    l_b, u_b, s_b, _, _ = _run_steps(dev, cfg, hbs, steps, dict(enabled=False), False)
    l_g, u_g, s_g, st, kinds = _run_steps(dev, cfg, hbs, steps, dict(bucket=dict(rows=quanta[0], scored=quanta[1]), warm_steps=warm), False)
    replays_salt = int(hip.dropout_salt(dev).item()) - salt0
    hip.dropout_salt(dev).zero_()
    noise_l = max(abs(a - b) / abs(a) for a, b in zip(l_a, l_b))
    got_l = max(abs(a - g) / abs(a) for a, g in zip(l_a, l_g))
    noise, got = _upd_rel(u_b, u_a), _upd_rel(u_g, u_a)
    print("quanta", quanta, "first seed", first, "kinds", kinds)
    print("quanta", quanta, "captures", st.captures, "signatures", st.signatures, "replays", st.replays, "eager", st.eager_steps)
    print("losses eager", l_a, "bucketed", l_g)
    print("loss rel: eager/eager %.3e bucketed/eager %.3e; update rel L2: eager/eager %.3e bucketed/eager %.3e" % (noise_l, got_l, noise, got))
    assert st.last_error is None, st.last_error
    if quanta == (1024, 256):
        assert st.captures == 1 and st.signatures == 1, (st.captures, st.signatures)
        assert st.eager_steps == warm and st.replays == steps - warm, (st.eager_steps, st.replays)
    else:
        assert 1 <= st.captures <= 2 and st.signatures <= 2, (st.captures, st.signatures)
        assert st.captures == st.signatures == (1 if first == 40 else 2), (st.captures, st.signatures)
        last_capture = max(i for i, k in enumerate(kinds) if k[2])
        assert all(k == (1, 0, 0) for k in kinds[last_capture + 1:]) and kinds[last_capture][0] == 1, kinds
        assert st.eager_steps == warm * st.signatures and st.replays == steps - st.eager_steps, (st.eager_steps, st.replays, kinds)
    assert replays_salt == st.replays
    assert s_a == s_g == {steps}, (s_a, s_g)
    assert got_l < 2e-5 + 4 * noise_l, (got_l, noise_l)
    assert got < max(1e-2, 2 * noise), (got, noise)
    # not the previous batch's data: the eight losses of the last cycle differ, and each replayed loss is nearer to the eager loss
    # of its own batch than to that of the batch before it
    cyc_g = l_g[16:24]
    assert max(cyc_g) - min(cyc_g) > 1e-3 * abs(cyc_g[0]), cyc_g
    for i in range(17, 24):
        if abs(l_a[i] - l_a[i - 1]) > 1e-3 * abs(l_a[i]):
            assert abs(l_g[i] - l_a[i]) < abs(l_g[i] - l_a[i - 1]), (i, l_g[i], l_a[i], l_a[i - 1])


def test_bucketed_step_with_dropout_and_wra(dev):
    """dropout 0.1 and the word-region alignment loss on (phrase_index kept; every device-side draw inside the capture): 16 steps
    over the eight batches.  Finite losses, the dropout salt advanced once per replay, final loss within 10 % of the eager run's
    (the criterion of test_graphed_step_matches_eager_steps for this variant)."""
    from mvp_pytorch_amd import hip
    cfg = dict(gu.TINY_CFG, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, max_phrases=3)
    hbs = _host_batches(cfg)
    steps = 16
    salt0 = int(hip.dropout_salt(dev).item())
    l_a, _, s_a, _, _ = _run_steps(dev, cfg, hbs, steps, dict(enabled=False), True)
    assert int(hip.dropout_salt(dev).item()) == salt0
    l_g, _, s_g, st, _ = _run_steps(dev, cfg, hbs, steps, dict(bucket=True), True)
    salt1 = int(hip.dropout_salt(dev).item())
    hip.dropout_salt(dev).zero_()
    print("eager", l_a, "bucketed", l_g, "captures", st.captures, "replays", st.replays)
    assert st.last_error is None, st.last_error
    assert st.captures == 1 and st.signatures == 1 and st.replays == steps - 2 and st.eager_steps == 2
    assert salt1 == salt0 + st.replays
    assert s_a == s_g == {steps}
    assert all(np.isfinite(l_g)) and abs(l_g[-1] - l_a[-1]) / abs(l_a[-1]) < 0.1, (l_g[-1], l_a[-1])


# ------------------------------------------------------------------------------------------------------------------------
def test_check_bounds_reports_through_the_error_word(dev):
    """hip.check_bounds alone, on hand-made count tensors (no model step runs with counts above its buffers): counts within the
    bounds leave the error word clear; one above its bound makes check_device_errors raise RuntimeError naming found and bound;
    the word is clear again afterwards; the first error wins."""
    from mvp_pytorch_amd import hip
    hip.check_device_errors(dev)
    a = torch.tensor([100, 12], dtype=torch.int64, device=dev)
    b = torch.tensor([90, 11], dtype=torch.int64, device=dev)
    hip.check_bounds(a, b, (100, 12, 90, 11))
    hip.check_bounds(a, b, (128, 15, 96, 11))
    hip.check_device_errors(dev)
    hip.check_bounds(a, b, (128, 15, 64, 11))           # rows_b = 90 > 64
    hip.check_bounds(a, b, (96, 15, 96, 11))            # a second overrun: the first one stays in the word
    with pytest.raises(RuntimeError, match=r"bound this pass was sized for.*found 90, bound 64"):
        hip.check_device_errors(dev)
    hip.check_device_errors(dev)
    hip.check_bounds(a, b, (128, 10, 96, 11))           # longest text sequence 12 > 10
    with pytest.raises(RuntimeError, match=r"found 12, bound 10"):
        hip.check_device_errors(dev)
    hip.check_device_errors(dev)


def test_captured_step_with_too_few_scored_slots_raises_at_the_next_call(dev, request):
    """A bounded captured step (the caller's own bounds in host_counts) replayed on a batch with two more scored text rows than
    the graph has slots: the step finishes with a finite loss (the surplus rows drop out of the loss, nothing is out of bounds),
    the NEXT call raises RuntimeError("... more scored ...") before it steps, the process lives, and the step after that works."""
    from mvp_pytorch_amd import dp, hip, modeling, train
    from mvp_pytorch_amd.modeling.modeling_vlbert import BOUND_KEYS
    from mvp_pytorch_amd.optimization import AdamW, WarmupLinearSchedule
    from mvp_pytorch_amd.synthetic import synthetic_batch
    cfg = dict(gu.TINY_CFG, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, max_phrases=3)
    _pin_randperm(request, dev)
    hbs = {s: synthetic_batch(DIMS, cfg, s) for s in (41, 46, 43)}
    big = int(hbs[43]["host_counts"]["scored_a"])
    slots = big - 2
    assert all(int(hbs[s]["host_counts"]["scored_a"]) <= slots for s in (41, 46)) and slots >= 1
    bounds = (240, 176, slots, 176)

    def on_dev(s):
        hb = hbs[s]
        out = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in hb.items() if k not in ("phrase_index", "image_index")}
        out["host_counts"] = type(hb["host_counts"])(hb["host_counts"], **dict(zip(BOUND_KEYS, bounds)))
        return out

    torch.manual_seed(0)
    model = modeling.BiBertImgForPreTraining(modeling.make_config(cfg)).to(dev)
    model.train()
    opt = AdamW([{"params": list(model.parameters()), "weight_decay": 0.01}], lr=1e-3, eps=1e-8)
    sync = dp.GradSync(model)
    stepper = train.GraphedStep(model, opt, WarmupLinearSchedule(opt, warmup_steps=10, t_total=100), max_tag_length=DIMS["G"],
                                max_grad_norm=1.0, grad_sync=sync, bucket=True)
    hip.check_device_errors(dev)
    for s in (41, 46, 41, 46):
        assert np.isfinite(float(stepper(on_dev(s))))
    stepper.check()
    assert stepper.last_error is None and stepper.captures == 1 and stepper.replays == 2 and stepper.signatures == 1
    loss = float(stepper(on_dev(43)))                   # 2 scored rows more than slots: a replay of the same graph
    assert np.isfinite(loss) and stepper.replays == 3
    with pytest.raises(RuntimeError, match="more scored"):
        stepper(on_dev(41))
    assert stepper.replays == 3                         # the raising call did not step
    assert np.isfinite(float(stepper(on_dev(41)))) and stepper.replays == 4
    loss = float(stepper(on_dev(43)))
    assert np.isfinite(loss)
    with pytest.raises(RuntimeError, match=r"more scored.*%d scored rows, %d slots" % (big, slots)):
        stepper.check()
    stepper.check()
    hip.check_device_errors(dev)
    sync.close()
