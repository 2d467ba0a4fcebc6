"""BiImageBertForSequenceClassificationPlus on MI355X: the feature-fusion kernels (csrc/fusion.hip) and the ReLU epilogue of
mvptr_sgemm_small against float64 / exact torch restatements, the fused head with replayed dropout masks against float64,
the whole model against the reference fixture (tests/golden/tiny_plus.npz) and the read-back-free captured step.

Measured values: profiles/r08_parity_values.txt."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as gu

pytestmark = pytest.mark.gpu

# the project's bounds (tests/test_model_gpu.py), copied
LOSS_RTOL = 1e-3            # target for losses
SMALL_ROWS_RTOL = 3e-3      # hard bound for losses over B = 4 rows
CEILING = {"logits": 0.04, "grad": 0.06}

U = 2.0 ** -24              # unit roundoff of f32
M32 = 0xFFFFFFFF
CAT2, PAIR4 = 0, 1


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def _keep(n, drop, salt=0):
    """The documented keep mask of n elements for a hip.Dropout (None: all kept), seeds mixed with the salt word as mvptr.h states."""
    if drop is None:
        return np.ones(n, dtype=np.float64), 1.0
    lo = (drop.seed_lo ^ ((salt * 0x9E3779B9) & M32)) & M32
    hi = (drop.seed_hi + salt * 0x85EBCA6B) & M32
    return gu.dropout_keep_np(n, lo, hi, drop.thresh16).astype(np.float64), 65536.0 / (65536.0 - drop.thresh16)


def _view(rows, cols, off, g, dev):
    """A random-normal [rows, cols] f32 view at column `off` of a wider tensor (row stride > cols)."""
    wide = torch.randn(rows, cols + 8, generator=g).to(dev)
    return wide[:, off:off + cols]


def _segments(a, b, mode):
    return [a, b, b - a, b * a] if mode == PAIR4 else [a, b]


def _check_features(dev, mode, rows, P, p, off, salt=0):
    from mvp_pytorch_amd import hip
    g = torch.Generator().manual_seed(1000 * rows + P + 7 * mode)
    nseg = 4 if mode == PAIR4 else 2
    W = nseg * P
    a, b, dout = _view(rows, P, off, g, dev), _view(rows, P, off, g, dev), _view(rows, W, off, g, dev)
    assert a.stride(0) > P and dout.stride(0) > W
    drop = hip.make_dropout(p, 0x9ABCDEF012345678 + rows) if p > 0 else None
    out = hip.fuse_features_fwd(a, b, mode, drop)
    da, db = hip.fuse_features_bwd(a, b, dout, mode, drop)
    torch.cuda.synchronize()
    keep, scale = _keep(rows * W, drop, salt)
    keep = keep.reshape(rows, W)
    a64, b64, d64 = a.double().cpu().numpy(), b.double().cpu().numpy(), dout.double().cpu().numpy()
    ref = np.concatenate(_segments(a64, b64, mode), 1) * keep * scale
    got = out.double().cpu().numpy()
    assert got.shape == (rows, W)
    assert np.array_equal(got != 0, keep != 0)                       # the mask, bit for bit (no input value is exactly 0)
    if p > 0 and rows * W > 2000:
        assert abs(keep.mean() - (1 - p)) < 0.03
    e_f = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300) * (keep != 0)
    assert e_f.max() <= 4 * U, e_f.max()
    gs = [keep[:, s * P:(s + 1) * P] * scale * d64[:, s * P:(s + 1) * P] for s in range(nseg)]
    if mode == PAIR4:
        da_ref, db_ref = gs[0] - gs[2] + gs[3] * b64, gs[1] + gs[2] + gs[3] * a64
        da_mag, db_mag = np.abs(gs[0]) + np.abs(gs[2]) + np.abs(gs[3] * b64), np.abs(gs[1]) + np.abs(gs[2]) + np.abs(gs[3] * a64)
    else:
        da_ref, db_ref, da_mag, db_mag = gs[0], gs[1], np.abs(gs[0]), np.abs(gs[1])
    e_a, e_b = np.abs(da.double().cpu().numpy() - da_ref), np.abs(db.double().cpu().numpy() - db_ref)
    assert (e_a <= 8 * U * scale * da_mag).all() and (e_b <= 8 * U * scale * db_mag).all(), \
        ((e_a / np.maximum(da_mag, 1e-300)).max() / U, (e_b / np.maximum(db_mag, 1e-300)).max() / U)
    return float(e_f.max() / U)


# (rows, P): odd P with an element pair that straddles two segments; P % 4 != 0 over more than one lane group (element-wise path);
# the tiny width and the real width on the 16-byte path (the view starts at a 16-byte boundary: off = 4); off = 1: a 16-byte-able
# shape behind a misaligned base
SHAPES = [(1, 3, 4), (5, 130, 4), (4, 128, 4), (33, 768, 4), (4, 128, 1)]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("rows,P,off", SHAPES)
@pytest.mark.parametrize("mode", [CAT2, PAIR4])
def test_fuse_features_against_float64(dev, mode, rows, P, off, p):
    worst = _check_features(dev, mode, rows, P, p, off)
    print("fuse_features mode %d rows %d P %d off %d p %.1f: forward error %.2f u" % (mode, rows, P, off, p, worst))


@pytest.mark.parametrize("rows,P", [(5, 130), (4, 128)])
def test_fuse_features_mix_the_salt_word_into_their_seeds(dev, rows, P):
    from mvp_pytorch_amd import hip
    word = hip.dropout_salt(dev)
    try:
        word.fill_(3)
        _check_features(dev, PAIR4, rows, P, 0.1, 4, salt=3)
        _check_features(dev, CAT2, rows, P, 0.1, 4, salt=3)
    finally:
        word.zero_()
        torch.cuda.synchronize()


@pytest.mark.parametrize("M,N,K", [(5, 70, 100), (33, 256, 512)])
def test_relu_epilogue_and_backward_are_exact(dev, M, N, K):
    from mvp_pytorch_amd import engine, hip
    g = torch.Generator().manual_seed(M + N)
    x, w, b = torch.randn(M, K, generator=g).to(dev), (torch.randn(N, K, generator=g) * K ** -0.5).to(dev), torch.randn(N, generator=g).to(dev)
    dy = torch.randn(M, N, generator=g).to(dev)
    plain = hip.sgemm_small(x, w, trans_b=True, bias=b, act=None)
    y = hip.sgemm_small(x, w, trans_b=True, bias=b, act="relu")
    assert torch.equal(y, plain.clamp_min(0))              # the same accumulator through one more max
    assert 0.2 < float((y > 0).float().mean()) < 0.8
    assert torch.equal(hip.relu_bwd(dy, y), dy * (y > 0))
    flat_dy, flat_y = dy.reshape(-1)[:M * N - 3], y.reshape(-1)[:M * N - 3]     # a length that is no multiple of 4
    assert torch.equal(hip.relu_bwd(flat_dy.contiguous(), flat_y.contiguous()), flat_dy * (flat_y > 0))
    off_dy, off_y = dy.reshape(-1)[1:], y.reshape(-1)[1:]                       # bases off the 16-byte grid
    assert torch.equal(hip.relu_bwd(off_dy, off_y), off_dy * (off_y > 0))
    grads = {}
    for act in ("relu", None):
        xs, ws, bs = (t.clone().requires_grad_(True) for t in (x, w, b))
        out = engine.SmallLinearFn.apply(xs, ws, bs, act, False)
        if act is None:
            out = torch.relu(out)
        assert torch.equal(out, y)
        out.backward(dy)
        grads[act] = (xs.grad, ws.grad, bs.grad)
    for got, ref in zip(grads["relu"], grads[None]):
        assert got is not None and torch.equal(got, ref)


def _plus_model(cfg, seed, dev, train):
    from mvp_pytorch_amd import modeling
    model = modeling.BiImageBertForSequenceClassificationPlus(modeling.make_config(cfg))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in gu.det_state_dict(shapes, seed).items()})
    model.to(dev)
    model.train(train)
    return model


def _head_params(model):
    return {n: p for n, p in model.named_parameters() if n.startswith(("single_mapping.", "classifier."))}


def _head_restated(params, pooled, gt, gi, keep4, keep2, scale):
    """The head from the formulas of include/mvptr.h and vl:2040-2045, in the dtype of its arguments, masks given."""
    def mlp(prefix, x):
        if prefix + ".weight" in params:
            return F.linear(x, params[prefix + ".weight"], params[prefix + ".bias"])
        h = torch.relu(F.linear(x, params[prefix + ".0.weight"], params[prefix + ".0.bias"]))
        return F.linear(h, params[prefix + ".2.weight"], params[prefix + ".2.bias"])
    x = torch.cat([gt, gi, gi - gt, gi * gt], 1) * keep4 * scale
    single = mlp("single_mapping", x)
    z = torch.cat([pooled, single], 1) * keep2 * scale
    return mlp("classifier", z)


@pytest.mark.parametrize("classifier,num_labels", [("linear", 3), ("mlp", 37)])
def test_fused_head_with_dropout_matches_float64_with_replayed_masks(dev, classifier, num_labels):
    """fuse_head in training mode with p = 0.1: the two seeds are pinned, the masks regenerated with the numpy restatement of the
    documented hash and replayed in an f64 restatement of the head.  Logits and the gradients of the three inputs and of every head
    parameter, by relative L2 against f64; the bound per quantity is 4x the error of the torch f32 composition of the same head
    (torch.cat, F.linear, the same masks) on the same device — the f32 MFMA GEMM adds four waves' partial sums, another summation
    order than the BLAS call's — with a floor of 2^-22."""
    from mvp_pytorch_amd import engine, hip
    p_drop, B = 0.1, 5
    cfg = dict(gu.TINY_CFG, hidden_dropout_prob=p_drop, attention_probs_dropout_prob=0.0, loss_type="ce", num_labels=num_labels,
               classifier=classifier)
    H = cfg["hidden_size"]
    model = _plus_model(cfg, 77, dev, train=True)
    g = torch.Generator().manual_seed(5)
    ins = [torch.randn(B, H, generator=g) for _ in range(3)]           # pooled, global_txt, global_img
    dy = torch.randn(B, num_labels, generator=g)
    seeds = [0x0123456789ABCDEF, 0xFEDCBA9876543210]
    it = iter(seeds)
    orig = engine.next_seed
    engine.next_seed = lambda: next(it)
    try:
        xs = [t.to(dev).requires_grad_(True) for t in ins]
        logits = model.fuse_head(*xs)
        logits.backward(dy.to(dev))
        torch.cuda.synchronize()
    finally:
        engine.next_seed = orig
    assert next(it, None) is None                                     # one seed per concat-and-dropout stage
    got = {"logits": logits.detach()}
    got.update({"d_" + n: x.grad for n, x in zip(("pooled", "global_txt", "global_img"), xs)})
    got.update({n: p.grad for n, p in _head_params(model).items()})
    assert all(v is not None for v in got.values())
    k4, scale = _keep(B * 4 * H, hip.make_dropout(p_drop, seeds[0]))
    k2, _ = _keep(B * 2 * H, hip.make_dropout(p_drop, seeds[1]))
    k4, k2 = torch.from_numpy(k4).view(B, 4 * H), torch.from_numpy(k2).view(B, 2 * H)

    def restated(dtype, device):
        ps = {n: p.detach().to(device=device, dtype=dtype).requires_grad_(True) for n, p in _head_params(model).items()}
        xin = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in ins]
        out = _head_restated(ps, *xin, k4.to(device=device, dtype=dtype), k2.to(device=device, dtype=dtype), scale)
        out.backward(dy.to(device=device, dtype=dtype))
        res = {"logits": out.detach()}
        res.update({"d_" + n: x.grad for n, x in zip(("pooled", "global_txt", "global_img"), xin)})
        res.update({n: p.grad for n, p in ps.items()})
        return res

    ref = restated(torch.float64, "cpu")
    base = restated(torch.float32, dev)
    worst = None
    for n in ref:
        e_hip, e_torch = _rel(got[n], ref[n]), _rel(base[n], ref[n])
        bound = max(4 * e_torch, 2.0 ** -22)
        print("PLUS head %s %s: hip %.3e torch-f32 %.3e bound %.3e" % (classifier, n, e_hip, e_torch, bound))
        if worst is None or e_hip / bound > worst[0]:
            worst = (e_hip / bound, n, e_hip, e_torch)
    assert worst[0] <= 1.0, worst
    # and the masks matter: without them the restatement is far away
    ones4, ones2 = torch.ones_like(k4), torch.ones_like(k2)
    ps = {n: p.detach().double().cpu() for n, p in _head_params(model).items()}
    assert _rel(got["logits"], _head_restated(ps, *[t.double() for t in ins], ones4, ones2, 1.0)) > 1e-2


@pytest.fixture(scope="module")
def plus():
    return gu.load("tiny_plus"), gu.load("tiny_finetune")


@pytest.mark.parametrize("tag", ["ve", "vqa"])
def test_plus_parity_with_reference(dev, plus, tag):
    d, ft = plus
    extra = json.loads(str(d[tag + "_cfg_json"]))
    cfg = dict(d["config"], hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, **extra)
    model = _plus_model(cfg, int(d["seed"]), dev, train=False)
    t = lambda k: torch.from_numpy(ft["in:" + k]).to(dev)  # noqa: E731
    kw = dict(input_ids_a=t("input_ids_a"), token_type_ids_a=t("segment_ids_a"), attention_mask_a=t("input_mask_a"),
              input_ids_b=t("input_ids_b"), token_type_ids_b=t("segment_ids_b"), attention_mask_b=t("input_mask_b"),
              img_feats=t("img_feats"))
    o = model(labels=torch.from_numpy(ft[tag + "_labels"]).to(dev), **kw)
    o[0].backward()
    torch.cuda.synchronize()
    e_loss = abs(o[0].item() - float(d[tag + "_loss"])) / float(d[tag + "_loss"])
    e_logits = _rel(o[1], torch.from_numpy(d[tag + "_logits"]))
    print("PARITY tiny_plus:%s loss %.3e (target %.0e: %s, bound %.0e) logits %.5f (bound %.2f)"
          % (tag, e_loss, LOSS_RTOL, "met" if e_loss < LOSS_RTOL else "MISSED", SMALL_ROWS_RTOL, e_logits, CEILING["logits"]))
    assert e_loss < SMALL_ROWS_RTOL
    assert e_logits < CEILING["logits"]
    names = [n for n in _head_params(model)] + ["bert.txt_proj", "bert.vis_proj"]
    assert len(names) == (6 if tag == "ve" else 8) + 2
    worst = (0.0, None)
    for n in names:
        p = dict(model.named_parameters())[n]
        ref = float(d["%s_gnorm:%s" % (tag, n)])
        assert p.grad is not None and ref > 0, n
        e = abs(p.grad.double().norm().item() - ref) / ref
        print("PARITY tiny_plus:%s gnorm %s %.5f" % (tag, n, e))
        worst = max(worst, (e, n))
    assert worst[0] < CEILING["grad"], worst


def test_plus_host_counts_and_captured_step(dev):
    """The `vqa` variant without read-backs (host_counts: bit-identical loss) and as a captured HIP graph (train.GraphedStep with a
    custom forward): forward, fused head, backward, clip and AdamW in one graph."""
    from mvp_pytorch_amd import dp, hip, train
    from mvp_pytorch_amd.optimization import AdamW, ConstantLRSchedule
    from mvp_pytorch_amd.synthetic import finetune_host_counts, synthetic_batch
    cfg = dict(gu.TINY_CFG, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, loss_type="bce", num_labels=37, classifier="mlp")
    dims = dict(B=10, T=18, P=3, G=20, R=8)
    b = {k: v.to(dev) for k, v in synthetic_batch(dims, cfg, 41).items() if isinstance(v, torch.Tensor)}
    kw = dict(input_ids_a=b["input_ids_a"], token_type_ids_a=b["segment_ids_a"], attention_mask_a=b["input_mask_a"],
              input_ids_b=b["input_ids_b"], token_type_ids_b=b["segment_ids_b"], attention_mask_b=b["input_mask_b"], img_feats=b["img_feats"])
    labels = torch.rand(dims["B"], 37, generator=torch.Generator().manual_seed(1)).to(dev)
    hc = finetune_host_counts(b, 20)
    got = {}
    for use_hc in (False, True):
        model = _plus_model(cfg, 23, dev, train=True)
        o = model(labels=labels, host_counts=hc if use_hc else None, **kw)
        o[0].backward()
        torch.cuda.synchronize()
        got[use_hc] = o[0].detach().clone()
    assert torch.equal(got[True], got[False])
    model = _plus_model(cfg, 23, dev, train=True)
    opt = AdamW([{"params": list(model.parameters()), "weight_decay": 0.01}], lr=1e-3, eps=1e-8)
    sync = dp.GradSync(model)
    try:
        step = train.GraphedStep(model, opt, ConstantLRSchedule(opt), max_grad_norm=1.0, grad_sync=sync, forward=lambda m, bb: m(**bb))
        vb = dict(kw, labels=labels, host_counts=hc)
        losses = [float(step(vb)) for _ in range(5)]
        torch.cuda.synchronize()
        print("PLUS captured step losses", losses, "eager", float(got[True]))
        assert step.last_error is None and step.captures == 1 and step.replays == 3, (step.last_error, step.captures, step.replays)
        assert abs(losses[0] - float(got[True])) < 1e-6 * abs(losses[0]) and losses[-1] < losses[0]
    finally:
        hip.dropout_salt(dev).zero_()
        sync.close()
