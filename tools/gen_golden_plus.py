#!/usr/bin/env python
"""Generate tests/golden/tiny_plus.npz: the REFERENCE's BiImageBertForSequenceClassificationPlus (vl:1975-2070, the
`--use_single` model of run_ve.py / run_vqa.py) on the inputs and labels of the tiny_finetune fixture (not stored again).
Runs only where tools/gen_golden.py runs (it imports the reference through that module's shims); the fixture holds the
reference's outputs and gradient summaries, no reference text.

Two variants, weights gu.det_state_dict(seed 1236 + 7), dropout 0, eval mode:
  ve    loss_type "ce",  num_labels 3,  classifier "linear"
  vqa   loss_type "bce", num_labels 37, classifier "mlp"

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_plus.py
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (installs the shims, imports the reference)

gu = gg.gu
ref_vl = gg.ref_vl

SEED = 1236 + 7
VARIANTS = {"ve": dict(loss_type="ce", num_labels=3, classifier="linear"),
            "vqa": dict(loss_type="bce", num_labels=37, classifier="mlp")}


def gen_plus(name="tiny_plus"):
    ft = gu.load("tiny_finetune")
    c, dims = ft["config"], ft["dims"]
    t = lambda k: torch.from_numpy(ft["in:" + k])  # noqa: E731
    # run_ve.py:515-523 / run_vqa.py:641-648 omit max_tag_length (default 20 = dims["G"])
    kw = dict(input_ids_a=t("input_ids_a"), token_type_ids_a=t("segment_ids_a"), attention_mask_a=t("input_mask_a"),
              input_ids_b=t("input_ids_b"), token_type_ids_b=t("segment_ids_b"), attention_mask_b=t("input_mask_b"),
              img_feats=t("img_feats"))
    data = {}
    for tag, extra in VARIANTS.items():
        cfg = dict(c, **extra)
        model = gg.load_det(ref_vl.BiImageBertForSequenceClassificationPlus(gg.make_config(cfg)), SEED)
        model.eval()
        taps = {}
        hooks = [model.single_mapping.register_forward_hook(lambda m, i, o: taps.__setitem__("single", o.detach().clone())),
                 model.bert.register_forward_hook(lambda m, i, o: taps.__setitem__("bert", o))]
        labels = torch.from_numpy(ft[tag + "_labels"])
        o = model(labels=labels, **kw)
        o[0].backward()
        for h in hooks:
            h.remove()
        outputs, single, _ = taps["bert"]
        gt = (single[0][:, 0, :] @ model.bert.txt_proj).detach()      # vl:2037-2038, un-normalised
        gi = (single[1][:, 0, :] @ model.bert.vis_proj).detach()
        data.update({tag + "_loss": np.array(o[0].item()), tag + "_logits": o[1].detach().numpy(),
                     tag + "_pooled_output": outputs[1].detach().numpy(), tag + "_global_txt": gt.numpy(),
                     tag + "_global_img": gi.numpy(), tag + "_single_hidden": taps["single"].numpy(),
                     tag + "_params_json": np.array(json.dumps([[k, list(v.shape)] for k, v in model.state_dict().items()])),
                     tag + "_cfg_json": np.array(gu.to_json(extra))})
        data.update({tag + "_" + k: v for k, v in gg.grad_summary(model).items()})
        print(name, tag, "loss %.6g" % o[0].item())
    data["config_json"] = np.array(gu.to_json(c))
    data["dims_json"] = np.array(gu.to_json(dims))
    data["seed"] = np.array(SEED)
    gu.save(name, data, gg.OUT)
    size = os.path.getsize(os.path.join(gg.OUT, name + ".npz"))
    assert size < gu.PART_BYTES and not os.path.exists(os.path.join(gg.OUT, name + ".part2.npz")), size
    print(name, "bytes", size)


if __name__ == "__main__":
    torch.set_num_threads(8)
    gen_plus()
