"""Host side of GraphedStep(bucket=...): bounds, the covering rule, the new exports, the replay copy-skip rule (no GPU)."""
import os
import re

import torch

import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = dict(B=16, T=12, P=3, G=6, R=5)
SEEDS = range(40, 48)


def _batches():
    from mvp_pytorch_amd.synthetic import synthetic_batch
    return [synthetic_batch(DIMS, gu.TINY_CFG, s) for s in SEEDS]


def test_bounds_cover_counts_and_the_covering_rule_makes_few():
    from mvp_pytorch_amd import train
    batches = _batches()
    caps = train.batch_caps(batches[0])
    assert caps == (16 * 15, 16 * 11, 16 * 15, 16 * 11)
    # quanta 32 / 8: plain rounding gives two distinct bounds for these seeds, so the covering rule can never need more
    quanta = train.bucket_quanta(dict(rows=32, scored=8))
    rounded, known, used = set(), [], []
    for b in batches:
        counts = tuple(int(b["host_counts"][k]) for k in train.COUNT_KEYS)
        plain = train.bucket_bounds(counts, caps, quanta)
        assert train.covers(plain, counts) and all(x <= c for x, c in zip(plain, caps)), (counts, plain)
        rounded.add(plain)
        bounds, created = train.cover_bounds(known, counts, caps, quanta)
        assert train.covers(bounds, counts) and all(x <= c for x, c in zip(bounds, caps)), (counts, bounds)
        assert created == (bounds not in used)
        used.append(bounds)
    assert rounded == {(192, 160, 24, 24), (192, 160, 32, 24)}, rounded
    assert 1 <= len(known) <= 2 and set(used) == set(known), known
    # fed smallest first the rule has to make both, and afterwards hands every batch the tightest bound that covers it
    known = []
    order = sorted(batches, key=lambda b: int(b["host_counts"]["scored_a"]))
    for b in order + order:
        counts = tuple(int(b["host_counts"][k]) for k in train.COUNT_KEYS)
        bounds, _ = train.cover_bounds(known, counts, caps, quanta)
        assert bounds == train.bucket_bounds(counts, caps, quanta)
    assert known == [(192, 160, 24, 24), (192, 160, 32, 24)]
    # a preferred (already captured) bound wins over a tighter one
    got, created = train.cover_bounds(list(known), (160, 150, 20, 20), caps, quanta, rank=lambda b: 0 if b == (192, 160, 32, 24) else 1)
    assert got == (192, 160, 32, 24) and not created
    # quanta 1024 / 256 (the defaults): the caps B*L decide, one bound for all eight
    quanta = train.bucket_quanta(True)
    assert quanta == (1024, 256)
    known = []
    for b in batches:
        counts = tuple(int(b["host_counts"][k]) for k in train.COUNT_KEYS)
        assert train.cover_bounds(known, counts, caps, quanta)[0] == (240, 176, 240, 176)
    assert known == [(240, 176, 240, 176)]
    # a count of zero still gets a buffer; a bad bucket argument is refused
    assert train.bucket_bounds((0, 0, 0, 0), caps, (32, 8)) == (32, 32, 8, 8)
    for bad in (dict(rows=0, scored=8), dict(rows=32, scored=8, other=1)):
        try:
            train.bucket_quanta(bad)
        except ValueError:
            continue
        raise AssertionError("accepted %r" % (bad,))


def test_check_bounds_is_exported_and_declared():
    from mvp_pytorch_amd import hip
    text = open(os.path.join(ROOT, "include", "mvptr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("mvptr_check_bounds", "mvptr_pack_maps_bounded"):
        assert name in hip.SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert "MVPTR_DEV_ERR_ROW_BOUND = 4" in text and hip.DEV_ERR_ROW_BOUND == 4
    assert "bound" in hip.DEV_ERR_TEXT[hip.DEV_ERR_ROW_BOUND]
    m = re.search(r"#define\s+MVPTR_ABI_VERSION\s+(\d+)", text)
    assert m and int(m.group(1)) == 7          # additive: the version stays


def test_replay_copies_unless_same_tensor_object():
    from mvp_pytorch_amd import train
    a = torch.arange(12).reshape(3, 4)
    note = (a, a._version)
    assert train.same_input(note, a)
    # another tensor at the same address with the same version (what a fresh batch on a reused allocation looks like)
    b = a.view(3, 4)
    assert b is not a and b.data_ptr() == a.data_ptr() and b._version == a._version
    assert not train.same_input(note, b)
    c = torch.as_strided(a, a.shape, a.stride())
    assert c is not a and (c.data_ptr(), c._version) == (a.data_ptr(), a._version)
    assert not train.same_input(note, c)
    assert not train.same_input(None, a)
    a.add_(1)                                   # the same object, written since the copy
    assert not train.same_input(note, a)
    assert train.same_input((a, a._version), a)


def test_bucketed_signature_leaves_the_counts_out():
    """two batches with different counts and the same bounds have one signature; without bucket= they have two (host logic only:
    a tensor subclass that claims to be on the device stands in for device tensors)"""
    from mvp_pytorch_amd import train
    from mvp_pytorch_amd.modeling.modeling_vlbert import BOUND_KEYS

    class Fake(torch.Tensor):
        is_cuda = True

    def fake(batch):
        return {k: (v.as_subclass(Fake) if torch.is_tensor(v) else v) for k, v in batch.items()}

    class M:
        training = True

    b0, b1 = (fake(b) for b in _batches()[:2])
    assert dict(b0["host_counts"]) != dict(b1["host_counts"])
    exact = train.GraphedStep(M(), None, None)
    assert exact.quanta is None and exact._signature(b0) != exact._signature(b1)
    st = train.GraphedStep(M(), None, None, bucket=True)
    o0, s0 = st._bound(b0)
    o1, s1 = st._bound(b1)
    assert s0 == s1 and st.signatures == 1
    assert tuple(o0["host_counts"][k] for k in BOUND_KEYS) == (240, 176, 240, 176)
    assert o1["host_counts"]["rows_a"] == b1["host_counts"]["rows_a"] and BOUND_KEYS[0] not in b1["host_counts"]
    # bounds the caller put into host_counts are kept
    own = dict(b1, host_counts=type(b1["host_counts"])(b1["host_counts"], **dict(zip(BOUND_KEYS, (200, 170, 40, 30)))))
    o2, s2 = st._bound(own)
    assert s2 != s1 and st.signatures == 2 and o2["host_counts"][BOUND_KEYS[2]] == 40
