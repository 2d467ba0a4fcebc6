"""BiImageBertForSequenceClassificationPlus on the host: parameter tree, and the torch composition of its head (the CPU /
model.half() path of fuse_head) against the reference's recorded activations (tests/golden/tiny_plus.npz, written by
tools/gen_golden_plus.py; inputs and labels are those of tiny_finetune).  f32 torch against the reference's f32 torch:
relative L2 <= 1e-5."""
import ctypes
import json

import pytest
import torch

import golden_util as gu

VARIANTS = ("ve", "vqa")
HOST_RTOL = 1e-5


@pytest.fixture(scope="module")
def plus():
    return gu.load("tiny_plus")


def _model(d, tag, **over):
    from mvp_pytorch_amd import modeling
    cfg = dict(d["config"], hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, **json.loads(str(d[tag + "_cfg_json"])))
    cfg.update(over)
    model = modeling.BiImageBertForSequenceClassificationPlus(modeling.make_config(cfg))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in gu.det_state_dict(shapes, int(d["seed"])).items()})
    return model.eval()


def _rel(a, b):
    a, b = a.double(), torch.as_tensor(b).double()
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("tag", VARIANTS)
def test_parameter_tree_equals_reference(plus, tag):
    from mvp_pytorch_amd import modeling
    cfg = dict(plus["config"], **json.loads(str(plus[tag + "_cfg_json"])))
    got = [[k, list(v)] for k, v in modeling.param_shapes("BiImageBertForSequenceClassificationPlus", cfg).items()]
    ref = json.loads(str(plus[tag + "_params_json"]))
    assert sorted(got) == sorted(ref)
    names = [k for k, _ in got]
    assert "single_mapping.0.weight" in names and "single_mapping.2.bias" in names
    assert ("classifier.weight" in names) == (tag == "ve") and ("classifier.2.weight" in names) == (tag == "vqa")


def test_classifier_without_config_attribute_is_built_like_the_reference(plus):
    from mvp_pytorch_amd import modeling
    cfg = dict(plus["config"], num_labels=3)
    assert "classifier" not in cfg
    shapes = modeling.param_shapes("BiImageBertForSequenceClassificationPlus", cfg)
    H = cfg["hidden_size"]
    assert shapes["classifier.weight"] == (3, H) and shapes["single_mapping.0.weight"] == (2 * H, 4 * H)


def test_text_only_config_raises(plus):
    from mvp_pytorch_amd import modeling
    cfg = dict(plus["config"], img_feature_dim=0, classifier="linear", num_labels=3)
    with pytest.raises(NotImplementedError):
        modeling.BiImageBertForSequenceClassificationPlus(modeling.make_config(cfg))


@pytest.mark.parametrize("tag", VARIANTS)
def test_cpu_head_reproduces_reference_activations_and_loss(plus, tag):
    """Pins the concat orders [t, i, i - t, i * t] and [pooled, single], and the loss."""
    from mvp_pytorch_amd.modeling.modeling_vlbert import _cls_loss
    model = _model(plus, tag)
    pooled, gt, gi = (torch.from_numpy(plus[tag + "_" + k]) for k in ("pooled_output", "global_txt", "global_img"))
    with torch.no_grad():
        single = model.single_hidden(gt, gi)
        logits = model.fuse_head(pooled, gt, gi)
        loss = _cls_loss(model, logits, torch.from_numpy(gu.load("tiny_finetune")[tag + "_labels"]), False)
    e_s, e_l = _rel(single, plus[tag + "_single_hidden"]), _rel(logits, plus[tag + "_logits"])
    e_loss = abs(loss.item() - float(plus[tag + "_loss"])) / float(plus[tag + "_loss"])
    print("plus host %s: single %.2e logits %.2e loss %.2e" % (tag, e_s, e_l, e_loss))
    assert e_s <= HOST_RTOL and e_l <= HOST_RTOL and e_loss <= HOST_RTOL
    # the orders matter: swapping the two global embeddings is far away
    with torch.no_grad():
        assert _rel(model.single_hidden(gi, gt), plus[tag + "_single_hidden"]) > 100 * HOST_RTOL


def test_head_refuses_a_classifier_of_the_wrong_width(plus):
    model = _model(plus, "ve")
    H = plus["config"]["hidden_size"]
    model.classifier = type(model.classifier)(H, 3)      # what the reference builds without config.classifier (vl:2009)
    with pytest.raises(RuntimeError):
        model.fuse_head(torch.zeros(2, H), torch.zeros(2, H), torch.zeros(2, H))


def test_new_entry_points_validate_before_any_launch():
    """Argument validation happens on the host before any launch: safe without a GPU (the pointers are never followed)."""
    import os
    from mvp_pytorch_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = hip.load()
    x = ctypes.c_void_p(4096)
    assert lib.mvptr_fuse_features_fwd(x, 8, x, 8, 0, 8, 0, None, x, 16, None) == -1 and b"fuse_features_fwd" in lib.mvptr_last_error()
    assert lib.mvptr_fuse_features_fwd(x, 8, x, 8, 2, 0, 0, None, x, 16, None) == -1      # P < 1
    assert lib.mvptr_fuse_features_fwd(x, 8, x, 8, 2, 8, 2, None, x, 16, None) == -1      # unknown mode
    assert lib.mvptr_fuse_features_fwd(x, 8, x, 8, 2, 8, 1, None, x, 16, None) == -1      # ldo < 4 P
    assert lib.mvptr_fuse_features_fwd(x, 8, None, 8, 2, 8, 0, None, x, 16, None) == -1   # NULL operand
    assert lib.mvptr_fuse_features_bwd(x, 8, x, 8, x, 16, 2, 8, 0, None, x, 4, x, 8, None) == -1 and b"fuse_features_bwd" in lib.mvptr_last_error()
    assert lib.mvptr_relu_bwd(x, x, x, 0, None) == -1 and b"relu_bwd" in lib.mvptr_last_error()
    assert lib.mvptr_relu_bwd(x, None, x, 8, None) == -1
    assert lib.mvptr_sgemm_small(x, 8, 0, 0, None, x, 8, 0, 1, None, 2, 2, 8, 1.0, None, 3, 0, x, 8, None) == -6      # act 3
    assert b"activation" in lib.mvptr_last_error()
    assert hip.SGEMM_ACT == {None: 0, "tanh": 1, "relu": 2}
