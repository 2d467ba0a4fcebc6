"""LayerNorm, attention and one BERT-base encoder layer against float64 at the row and item counts of the pre-training step.

The op tests of test_ops_gpu.py stop below the code paths the step runs (M <= 1 000 LayerNorm rows, <= 144 attention
items), and the step-size tests of test_model_gpu.py compare the HIP path with itself.  Here every expected value is plain
torch in float64 on the same bf16-rounded inputs the kernels read; nothing from mvp_pytorch_amd.hip computes one, except
hip.dropout_mask once test_dropout_hash_matches_documented_formula has pinned it to the formula of include/mvptr.h.

Every check is per unit (row, (sequence, head), weight row, column), because a global relative L2 cannot see one bad unit
among tens of thousands: one wrong row of 37 748 moves it by sqrt(1 / 37 748) = 5.1e-3.  Each test carries a negative
control built from its own float64 reference: a one-unit defect that exceeds the per-unit bound by at least 5x while it stays
under the global bound the suite used before.

Bounds are about 2x the worst value measured on an MI355X (quoted per test), never looser than the op test's bound for the
same quantity.

Step sizes (pre-training step at BASELINE configs[1]): valid rows of the three encoder passes 10 917 (text),
11 143 (visual) and 37 748 (joint, ~512 sequences of 20 - 125 rows, 12 heads).
"""
import math

import pytest
import torch

import golden_util as gu
from oracle import mvptr_oracle as orc

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _bf(x):
    return x.to(torch.bfloat16)


def _unit_rel(got, ref, seg=None, n=None, floor=0.0):
    """got, ref [R, K, C]: per-unit ||got - ref|| / (||ref|| + floor) in float64, the unit being (seg[r], k) (seg None: (r, k))
    and the C elements reduced -> ([n or R, K] errors, global relative L2 over everything)."""
    got, ref = got.to(F64), ref.to(F64)
    d2 = (got - ref).square().sum(-1)
    r2 = ref.square().sum(-1)
    if seg is not None:
        d2 = torch.zeros((n,) + d2.shape[1:], dtype=F64, device=d2.device).index_add_(0, seg, d2)
        r2 = torch.zeros((n,) + r2.shape[1:], dtype=F64, device=r2.device).index_add_(0, seg, r2)
    per = d2.sqrt() / (r2.sqrt() + floor)
    glob = math.sqrt(float(d2.sum()) / float(r2.sum()))
    return per, glob


def _col_rel(got, ref):
    """1-D gradients (per column / per element): |got - ref| / rms(ref) -> (per element, global relative L2)."""
    got, ref = got.to(F64).reshape(-1), ref.to(F64).reshape(-1)
    rms = ref.square().mean().sqrt()
    return (got - ref).abs() / rms, float((got - ref).norm() / ref.norm())


def _report(name, per, glob, bound):
    per = per.reshape(-1).float()
    worst, med = float(per.max()), float(per.median())
    print("%-28s worst %.3e  median %.3e  global %.3e  bound %.1e" % (name, worst, med, glob, bound))
    return worst


def _check(name, per, glob, bound):
    worst = _report(name, per, glob, bound)
    assert worst < bound, (name, worst, bound)


def _control(name, per_bad, glob_bad, bound, old_global=None):
    """negative control: the one-unit defect breaks the per-unit bound >= 5x and (old_global given) passes the old global bound"""
    worst = float(per_bad.max())
    print("%-28s control: defect unit %.3e (%.0fx bound)  global %.3e (old bound %s)" % (name, worst, worst / bound, glob_bad, old_global))
    assert worst >= 5 * bound, (name, worst, bound)
    assert old_global is None or glob_bad < old_global, (name, glob_bad, old_global)


def _zero_salt(dev):
    from mvp_pytorch_amd import hip
    hip.dropout_salt(dev).zero_()     # a graph-replayed step earlier in the process leaves its replay count in the word


def _dropout(seed, thresh16):
    from mvp_pytorch_amd import hip
    d = hip.Dropout()
    d.seed_lo, d.seed_hi, d.thresh16, d.pad_ = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, thresh16, 0
    return d


# ------------------------------------------------------------------------------------------------------------ 1. dropout hash

@pytest.mark.parametrize("thresh16", [1, 6554, 32768, 65535])
def test_dropout_hash_matches_documented_formula(dev, thresh16):
    """hip.dropout_mask (mvptr_dropout_mask) against gu.dropout_keep_np, a numpy restatement of the hash documented at
    mvptr_dropout in include/mvptr.h, bit for bit over n = 1 000 003 elements (odd n: the last hash pair is half used).  Every
    other dropout expectation in the suite is built with hip.dropout_mask, so this pins them all to the documentation.
    (n < 2^33, so the (j >> 32) * 0x9E3779B9 term is zero here: no test can afford a mask of 2^33 elements.)
    Kept-value scale 65536 / (65536 - thresh16): the identity-mode LayerNorm (gamma = NULL, y = dropout(z)) of both kernel
    families, the H = 768 one and the generic one, must give bf16(z * scale) on kept elements (within half a bf16 ulp of
    the float64 product) and exactly 0 elsewhere.
    Negative control: the restatement with thresh16 + 1 differs from the kernel's mask exactly on the elements whose u16 is
    thresh16 (a bit-level comparison, so any single-element difference fails)."""
    from mvp_pytorch_amd import hip
    _zero_salt(dev)
    n = 1_000_003
    seed = 0x8F3A_51C7_0B2E_D964
    d = _dropout(seed, thresh16)
    got = hip.dropout_mask(d, n, dev).cpu().numpy()
    want = gu.dropout_keep_np(n, d.seed_lo, d.seed_hi, thresh16)
    bad = int((got != want).sum())
    print("thresh16 %d: keep rate %.5f (expected %.5f), %d mismatches" % (thresh16, got.mean(), 1 - thresh16 / 65536, bad))
    assert bad == 0
    assert abs(float(got.mean()) - (1 - thresh16 / 65536)) < 5 * math.sqrt(thresh16 / 65536 * (1 - thresh16 / 65536) / n) + 1e-6
    if thresh16 < 65535:
        off = gu.dropout_keep_np(n, d.seed_lo, d.seed_hi, thresh16 + 1)
        assert (off != got).any()
    scale = 65536.0 / (65536.0 - thresh16)
    g = torch.Generator().manual_seed(thresh16)
    for H in (768, 128):
        M = 8192 // H * 64
        z = _bf(torch.randn(M, H, generator=g))
        y, _, _ = hip.layernorm_fwd(z.to(dev), None, None, 0.0, drop=d, save_stats=False)
        y = y.cpu().to(F64)
        keep = torch.from_numpy(gu.dropout_keep_np(M * H, d.seed_lo, d.seed_hi, thresh16)).reshape(M, H).bool()
        ref = z.to(F64) * scale
        assert torch.all(y[~keep] == 0)
        err = (y - ref).abs()[keep]
        assert torch.all(err <= _half_ulp(ref[keep])), (H, float(err.max()))


# ------------------------------------------------------------------------------------------------------------ 2. LayerNorm

def _half_ulp(v):
    """half a bf16 ulp of |v| (8 significant bits): 2^(e - 9) with |v| = m 2^e, m in [0.5, 1)"""
    _, e = torch.frexp(v.abs())
    return torch.ldexp(torch.ones_like(v), e - 9)


# Launch constants (csrc/rowops.hip):
#   H = 768 forward  ln_fwd_j_kernel<3, 2>: <= 2 048 blocks x 4 waves x 2 rows -> a pass covers 16 384 rows, then grid-strides.
#   H = 768 backward ln_bwd_j_kernel<3, 2, true>: <= 512 blocks x 4 waves x 2 rows -> 4 096 rows per pass; wave w's row sets
#     start at 2 w + 4 096 k and alternate between register sets A (k even) and B (k odd), the next set loading while the
#     current one finishes.
#   generic forward ln_fwd_kernel: <= 2 048 blocks x 4 waves x 1 row (8 192 rows per pass);
#   generic backward ln_bwd_kernel: <= 512 blocks x 4 waves x 1 row (2 048 rows per pass).
# M values, H = 768:
#   4 095  one pass, the last wave's only set half full (r1 >= M right away);
#   4 097  wave 0 has a second set of one row, B (r1 < M <= r2); every other wave stops after A (r1 >= M);
#   8 193  wave 0 runs A, B and a third set of one row back in A; the others A, B: the pipeline's steady state;
#  12 288  every wave finishes on set A (three sets: A, B, A);
#  16 384  every wave finishes on set B (four sets: A, B, A, B) and the forward's first pass is exactly full;
#  16 385  one row past the forward pass: the forward grid-stride loop runs a second time (block 0, wave 0);
#  10 917  text rows of the step;  37 748  joint rows of the step (forward: three passes; backward: ten sets per wave).
# H = 128 and 1 024 (generic kernels): 4 097 (two backward passes, one row in the second), 8 193 (forward grid-stride loop,
# one row), 16 385, 37 748.
LN_CASES = [(768, m) for m in (4095, 4097, 8193, 12288, 16384, 16385, 10917, 37748)] + \
           [(h, m) for h in (128, 1024) for m in (4097, 8193, 16385, 37748)]

# bounds (per unit; measured MI355X worst in the docstring)
# bounds: about 2x the worst over all cases of both LayerNorm tests on an MI355X (measured worst / largest per-case median)
LN_Y_ATOL = 1e-6          # y: |y - y64| - half a bf16 ulp of y64, per element (3.9e-7 / 0: all but a few elements within half an ulp)
LN_MEAN = 2.5e-7          # |mean - mean64| * rstd64 per row (1.1e-7 / 6.3e-9)
LN_RSTD = 4e-7            # |rstd / rstd64 - 1| per row (1.8e-7 / 3.3e-8)
LN_DZ_ROW = 5e-3          # dz and dd per row, relative L2 (2.3e-3 / 1.7e-3; op test's global dz bound 6e-3)
LN_DCOL = 2.5e-6          # dgamma, dbeta per column / rms (1.1e-6 / 1.1e-7; op test's global bound 1e-3)
LN_DBIAS_COL = 2e-6       # dbias per column / rms (8.1e-7 / 1.2e-7; op test's global bound 5e-3)


def _ln_inputs(M, H, seed):
    g = torch.Generator().manual_seed(seed)
    # rows of varying location and scale, like a residual stream (and so that neighbouring rows' statistics differ)
    loc = torch.rand(M, 1, generator=g) - 0.5
    sc = torch.rand(M, 1, generator=g) * 0.7 + 0.7
    z = _bf(torch.randn(M, H, generator=g) * sc + loc)
    gamma = 1 + 0.1 * torch.randn(H, generator=g)
    beta = 0.1 * torch.randn(H, generator=g)
    dy = _bf(torch.randn(M, H, generator=g))
    return z, gamma, beta, dy


def _ln_ref(z, gamma, beta, dy, eps=1e-12, keep_y=None, keep_d=None):
    """float64 LayerNorm forward + backward via the oracle's layer_norm and autograd.  keep_y: dropout (keep * scale) on the
    output (the gradient arriving is dy * keep_y); keep_d: the masked copy dd = dz * keep_d."""
    zr = z.to(F64).requires_grad_(True)
    gr = gamma.to(F64).requires_grad_(True)
    br = beta.to(F64).requires_grad_(True)
    y = orc.layer_norm(zr, gr, br, eps)
    g = dy.to(F64) if keep_y is None else dy.to(F64) * keep_y
    y.backward(g)
    mu = zr.detach().mean(-1)
    rs = 1.0 / torch.sqrt((zr.detach() - mu[:, None]).square().mean(-1) + eps)
    dz = zr.grad
    dd = dz if keep_d is None else dz * keep_d
    return dict(y=y.detach(), mean=mu, rstd=rs, dz=dz, dd=dd, dgamma=gr.grad, dbeta=br.grad, dbias=dd.sum(0))


def _ln_check_rows(tag, got, ref, M, H):
    y, mean, rstd, dz, dd, dg, db, dbias = got
    exc = ((y.to(F64) - ref["y"]).abs() - _half_ulp(ref["y"])).clamp_min(0).amax(-1)
    _check(tag + " y excess/half-ulp", exc, 0.0, LN_Y_ATOL)
    if mean is not None:
        _check(tag + " mean", (mean.to(F64) - ref["mean"]).abs() * ref["rstd"], 0.0, LN_MEAN)
        _check(tag + " rstd", (rstd.to(F64) / ref["rstd"] - 1).abs(), 0.0, LN_RSTD)
    _check(tag + " dz/row", *_unit_rel(dz.view(M, 1, H), ref["dz"].view(M, 1, H)), LN_DZ_ROW)
    if dd is not None:
        _check(tag + " dd/row", *_unit_rel(dd.view(M, 1, H), ref["dd"].view(M, 1, H)), LN_DZ_ROW)
    if dg is not None:
        _check(tag + " dgamma/col", *_col_rel(dg, ref["dgamma"]), LN_DCOL)
    _check(tag + " dbeta/col", *_col_rel(db, ref["dbeta"]), LN_DCOL)
    _check(tag + " dbias/col", *_col_rel(dbias, ref["dbias"]), LN_DBIAS_COL)


@pytest.mark.parametrize("H,M", LN_CASES)
def test_layernorm_rows_at_step_sizes(dev, H, M):
    """mvptr_layernorm_fwd / _bwd at the step's row counts against float64: y element-wise within half a bf16 ulp + an
    absolute term, mean and rstd per row, dz per row, dgamma / dbeta / dbias per column (float64 sums over all M rows; the
    kernel's go through <= 512 partial rows and the 32-slice finalize).  M values: see LN_CASES above.
    Measured on an MI355X, worst / median over rows or columns, worst case of the 16: y beyond half an ulp 3.9e-7 / 0,
    mean 1.1e-7 / 6.3e-9, rstd 1.8e-7 / 3.3e-8, dz per row 2.2e-3 / 1.7e-3, dgamma 8.2e-7 / 1.1e-7, dbeta 6.0e-7 / 5.8e-8,
    dbias 8.0e-7 / 1.1e-7 per column; bounds LN_* above (about 2x, under the op tests' global bounds).
    Negative control (M = 37 748): the last row's dz computed from row M - 2's mean and rstd: 0.23 - 0.42 on that row
    (>= 45x LN_DZ_ROW), global relative L2 1.2e-3 - 2.8e-3, under the op test's 6e-3."""
    from mvp_pytorch_amd import hip
    z, gamma, beta, dy = _ln_inputs(M, H, 1000 * H + M)
    zd, gd, bd, dyd = z.to(dev), gamma.to(dev), beta.to(dev), dy.to(dev)
    y, mean, rstd = hip.layernorm_fwd(zd, gd, bd, 1e-12)
    dg, db, dbias = (torch.zeros(H, device=dev) for _ in range(3))
    dz, dd = hip.layernorm_bwd(dyd, zd, mean, rstd, gd, dg, db, dbias)
    assert dd is None
    ref = _ln_ref(zd, gd, bd, dyd)
    _ln_check_rows("ln H=%d M=%d" % (H, M), (y, mean, rstd, dz, None, dg, db, dbias), ref, M, H)
    if M == 37748:
        # the defect: row M-1 normalised with row M-2's statistics (forward), its gradient likewise
        zl = zd[-1:].to(F64)
        xh = (zl - ref["mean"][-2]) * ref["rstd"][-2]
        gx = dyd[-1:].to(F64) * gd.to(F64)
        dz_bad = ref["dz"].clone()
        dz_bad[-1:] = ref["rstd"][-2] * (gx - gx.mean(-1, keepdim=True) - xh * (gx * xh).mean(-1, keepdim=True))
        per, glob = _unit_rel(dz_bad.view(M, 1, H), ref["dz"].view(M, 1, H))
        _control("ln dz/row", per, glob, LN_DZ_ROW, 6e-3)


@pytest.mark.parametrize("H", [768, 128])
def test_layernorm_remap_and_dropout_at_joint_size(dev, H):
    """M = 37 748 rows with the row remap of the image-embedding LayerNorm (rows_per_group R = 50 rows of each group of
    group_stride = 70 rows, at row_offset = 20: the last group holds 37 748 - 754 x 50 = 48 rows) and both dropout sites:
    y_drop on the output (forward: element index m * H + n of the compact row m; backward: regenerated on dy), dense_drop
    (dd = dz * keep, the copy for the preceding dense layer; dbias sums dd).  Keep masks from hip.dropout_mask (pinned by
    test_dropout_hash_matches_documented_formula).  The remapped output and the gradient input are prefilled with a sentinel:
    no row outside the remap's image may be written, and every image row must be.
    Measured on an MI355X (worst / median, worse of H = 768 and 128): dz per row 2.3e-3 / 1.7e-3, dd per row 2.3e-3 / 1.7e-3,
    y beyond half an ulp 3.0e-7, dgamma 7.0e-7, dbeta 1.1e-6, dbias 8.1e-7 per column / rms; bounds LN_* (shared with the
    test above).
    Negative control: dd of the last row with the mask of row M - 2: 0.41 - 0.48 on that row (>= 80x LN_DZ_ROW), global
    relative L2 2.3e-3, under the op test's 6e-3."""
    from mvp_pytorch_amd import hip
    _zero_salt(dev)
    M, R, G = 37748, 50, 20
    S = R + G
    ng = -(-M // R)
    z, gamma, beta, dy_rows = _ln_inputs(M, H, 77 + H)
    zd, gd, bd = z.to(dev), gamma.to(dev), beta.to(dev)
    yd, ddp = hip.make_dropout(0.1, 0x5EED0001 + H), hip.make_dropout(0.1, 0x5EED0002 + H)
    sc = 65536.0 / (65536.0 - yd.thresh16)
    ky = hip.dropout_mask(yd, M * H, dev).view(M, H).to(F64) * sc
    kd = hip.dropout_mask(ddp, M * H, dev).view(M, H).to(F64) * sc
    m = torch.arange(M, device=dev)
    img = (m // R) * S + G + m % R                       # compact row -> remapped row
    sentinel = torch.tensor(-12345.0, dtype=torch.bfloat16)
    out = torch.full((ng * S, H), float(sentinel), dtype=torch.bfloat16, device=dev)
    _, mean, rstd = hip.layernorm_fwd(zd, gd, bd, 1e-12, out=out, rows_per_group=R, group_stride=S, row_offset=G, drop=yd)
    hit = torch.zeros(ng * S, dtype=torch.bool, device=dev)
    hit[img] = True
    assert torch.all(out[~hit] == sentinel), "rows outside the remap written"
    assert not torch.any(out[hit] == sentinel)
    dy_full = torch.full((ng * S, H), float(sentinel), dtype=torch.bfloat16, device=dev)
    dy_full[img] = dy_rows.to(dev)
    dg, db, dbias = (torch.zeros(H, device=dev) for _ in range(3))
    dz, dd = hip.layernorm_bwd(dy_full, zd, mean, rstd, gd, dg, db, dbias, rows_per_group=R, group_stride=S, row_offset=G,
                               y_drop=yd, dense_drop=ddp)
    ref = _ln_ref(zd, gd, bd, dy_rows.to(dev), keep_y=ky, keep_d=kd)
    ref["y"] = ref["y"] * ky
    _ln_check_rows("ln remap+drop H=%d" % H, (out[img], mean, rstd, dz, dd, dg, db, dbias), ref, M, H)
    dd_bad = ref["dd"].clone()
    dd_bad[-1] = ref["dz"][-1] * kd[-2]
    per, glob = _unit_rel(dd_bad.view(M, 1, H), ref["dd"].view(M, 1, H))
    _control("ln dd/row", per, glob, LN_DZ_ROW, 6e-3)


# ------------------------------------------------------------------------------------------------------------ 3. attention

# (sequences, shortest, Lmax = longest, seed): the kernel is chosen by Lp = Lmax rounded up to 32 (attention.hip, launch of the backward:
# Lp <= 96 fused occupancy-3, Lp 128 fused occupancy-2, longer two-pass).  One workgroup per (sequence, head) item; a
# persistent kernel would start looping over items past CUs x residents = 256 x 2-3 = 512-768 items, so every case has more.
ATTN_CASES = {
    "joint": (512, 20, 125, 1),     # 6 144 items, Lp 128 (the joint stack: ~37 k rows)
    "text": (256, 1, 75, 2),        # 3 072 items, Lp 96; includes one-row sequences
    "visual": (256, 20, 50, 3),     # 3 072 items, Lp 64
    "long": (96, 130, 256, 4),      # 1 152 items, Lp 256: two-pass kernels
}
HEADS = 12
# bounds: about 2x the worst over all eight runs on an MI355X (measured worst / largest per-run median)
ATTN_CTX = 6e-3          # ctx per (sequence, head), relative L2 (3.4e-3 / 2.3e-3; 2x is 6.8e-3, capped at the op tests' 6e-3)
ATTN_LSE = 2e-6          # lse per (sequence, head), max abs over the valid queries (8.7e-7 / 7.0e-7; op tests 2e-3)
ATTN_DQKV = 1e-2         # dQ / dK / dV per (sequence, head), relative L2 (5.1e-3 / 2.4e-3; op tests 1.5e-2)
ATTN_REL_FLOOR = 1e-3    # in every relative norm: a one-row sequence whose one key is dropped has ctx = dV = 0 exactly


def _attn_ref64(qkv_pad, add_mask, dctx_pad, heads, keep=None, scale=1.0):
    """float64 self-attention on the padded layout: qkv_pad [B, L, 3H], add_mask broadcastable to [B, heads, L, L],
    keep [B, heads, L, L] or None -> ctx [B, L, H], lse [B, heads, L], and the backward pass as the backward kernel defines it:
    its inputs are the FORWARD OUTPUT ctx (bf16) and dctx, and delta = rowsum(dctx * ctx) is taken from that ctx.  The ctx fed
    to it is bf16(float64 ctx), the one given to the kernel too -> dqkv [B, L, 3H].  With an exact ctx this is the gradient
    of the forward; with the bf16 one it differs by |dS| ~ 2^-9 |dO.V|, which is what test_attention_every_block_count_per_head
    allows 0.3 absolute per 64-element slice for (one-row sequences, whose exact dQ, dK are 0)."""
    B, L, _ = qkv_pad.shape
    q, k, v = qkv_pad.to(F64).view(B, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / 8.0 + add_mask
    p = torch.softmax(s, -1)
    pd = p if keep is None else p * keep * scale
    ctx = (pd @ v).permute(0, 2, 1, 3).reshape(B, L, heads * 64)
    ctx_in = ctx.to(torch.bfloat16).to(F64)
    do = dctx_pad.to(F64).view(B, L, heads, 64).permute(0, 2, 1, 3)
    o = ctx_in.view(B, L, heads, 64).permute(0, 2, 1, 3)
    dv = pd.transpose(-1, -2) @ do
    dp = do @ v.transpose(-1, -2)
    if keep is not None:
        dp = dp * keep * scale
    ds = p * (dp - (do * o).sum(-1, keepdim=True))
    dq = ds @ k / 8.0
    dk = ds.transpose(-1, -2) @ q / 8.0
    dqkv = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).reshape(B, L, 3 * heads * 64)
    return ctx, torch.logsumexp(s, -1), ctx_in, dqkv


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
@pytest.mark.parametrize("case", list(ATTN_CASES))
def test_attention_packed_items_at_step_sizes(dev, case, p_drop):
    """Row-packed attention forward + backward (mvptr_attention_fwd_packed / _bwd_packed) against float64 at the step's item
    counts: ctx and lse per (sequence, head), dQ, dK and dV per (sequence, head).  With dropout the keep mask is
    hip.dropout_mask at the documented element index ((b * heads + h) * Lmax + q) * Lp + key.
    The backward kernel reads the forward's outputs (ctx, lse); it is given the float64 forward's, ctx rounded to bf16 as the
    forward kernel stores it, and the float64 backward takes delta from the same bf16 ctx (_attn_ref64).  One-row sequences
    are then held to the same relative bound as the rest instead of the 0.3 absolute floor of the op test.
    Measured on an MI355X, worst / median per item over the eight runs: ctx 3.4e-3 / 2.3e-3, lse 8.7e-7 / 7.0e-7,
    dQ 5.1e-3 / 2.4e-3, dK 3.8e-3 / 2.3e-3, dV 3.7e-3 / 2.4e-3; bounds ATTN_* above.
    Negative control: sequence 0 (length Lmax), head 0, with its last 32-key block dropped (every key of the block masked):
    the item's dQKV error 0.37 - 0.77 (>= 36x ATTN_DQKV, ctx >= 60x ATTN_CTX) while the global relative L2 of dQKV stays at
    7.3e-3 - 1.3e-2, under the op tests' 1.5e-2.  (The same defect moves the global ctx error to 6.7e-3 - 1.5e-2, so it is
    not asserted against 6e-3.)"""
    from mvp_pytorch_amd import hip
    _zero_salt(dev)
    B, lo, Lmax, seed = ATTN_CASES[case]
    H = HEADS * 64
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(lo, Lmax + 1, (B,), generator=g)
    lens[0] = Lmax
    if lo == 1:
        lens[1:4] = 1
    rows = int(lens.sum())
    qkv = _bf(torch.randn(rows, 3 * H, generator=g)).to(dev)
    dctx = _bf(torch.randn(rows, H, generator=g)).to(dev)
    lens_d = lens.to(torch.int32).to(dev)
    starts = (torch.cumsum(lens_d, 0) - lens_d).to(torch.int32)
    seg = torch.repeat_interleave(torch.arange(B, device=dev), lens.to(dev))
    pad_idx = seg * Lmax + (torch.arange(rows, device=dev) - starts.long()[seg])
    drop = hip.make_dropout(p_drop, 0xA77E_0000 + B) if p_drop > 0 else None
    keep, scale = None, 1.0
    if drop is not None:
        Lp = (Lmax + 31) // 32 * 32
        keep = hip.dropout_mask(drop, B * HEADS * Lmax * Lp, dev).view(B, HEADS, Lmax, Lp)[..., :Lmax].to(F64)
        scale = 65536.0 / (65536.0 - drop.thresh16)
    ctx, lse = hip.attention_fwd_packed(qkv, starts, lens_d, B, Lmax, HEADS, drop=drop)

    def pad(t):
        out = torch.zeros(B * Lmax, t.shape[1], dtype=F64, device=dev)
        out[pad_idx] = t.to(F64)
        return out.view(B, Lmax, -1)

    valid = torch.zeros(B * Lmax, dtype=torch.bool, device=dev)
    valid[pad_idx] = True
    valid = valid.view(B, Lmax)
    add_mask = ((~valid).to(F64) * -10000.0)[:, None, None, :]
    qkv_pad, dctx_pad = pad(qkv), pad(dctx)
    ctx_r, lse_r, ctx_in, dqkv_r = _attn_ref64(qkv_pad, add_mask, dctx_pad, HEADS, keep, scale)
    ctx_r, dqkv_r = ctx_r.view(B * Lmax, H)[pad_idx], dqkv_r.view(B * Lmax, 3 * H)[pad_idx]
    # the backward kernel reads the forward's outputs: give it the float64 forward's, rounded as the kernel stores them
    ctx_in = ctx_in.view(B * Lmax, H)[pad_idx].to(torch.bfloat16).contiguous()
    dqkv = hip.attention_bwd_packed(qkv, starts, lens_d, ctx_in, dctx, lse_r.float().contiguous(), B, Lmax, HEADS, drop=drop)
    tag = "attn %s p=%.1f" % (case, p_drop)
    print("%s: %d sequences x %d heads = %d items, %d rows" % (tag, B, HEADS, B * HEADS, rows))
    _check(tag + " ctx/item", *_unit_rel(ctx.view(rows, HEADS, 64), ctx_r.view(rows, HEADS, 64), seg, B, ATTN_REL_FLOOR), ATTN_CTX)
    lse_err = torch.where(valid[:, None, :], (lse.to(F64) - lse_r).abs(), 0.0).amax(-1)
    _check(tag + " lse/item", lse_err, 0.0, ATTN_LSE)
    lens_dev = lens.to(dev)
    for i, part in enumerate("QKV"):
        got = dqkv.view(rows, 3, HEADS, 64)[:, i]
        want = dqkv_r.view(rows, 3, HEADS, 64)[:, i]
        per, glob = _unit_rel(got, want, seg, B, ATTN_REL_FLOOR)
        print("%s d%s: worst item in a sequence of %d rows" % (tag, part, int(lens_dev[per.max(1).values.argmax()])))
        _check(tag + " d%s/item" % part, per, glob, ATTN_DQKV)
    # negative control: sequence 0 (length Lmax), head 0, keys of the last 32-key block masked out
    m0 = add_mask[:1].expand(1, HEADS, 1, Lmax).clone()
    m0[0, 0, 0, (Lmax - 1) // 32 * 32:] = -10000.0
    c0, _, _, d0 = _attn_ref64(qkv_pad[:1], m0, dctx_pad[:1], HEADS, None if keep is None else keep[:1], scale)
    n0 = int(lens[0])
    ctx_bad, dqkv_bad = ctx_r.clone(), dqkv_r.clone()
    ctx_bad[:n0], dqkv_bad[:n0] = c0[0, :n0], d0[0, :n0]
    per, glob = _unit_rel(ctx_bad.view(rows, HEADS, 64), ctx_r.view(rows, HEADS, 64), seg, B, ATTN_REL_FLOOR)
    _control(tag + " ctx/item", per, glob, ATTN_CTX)
    per, glob = _unit_rel(dqkv_bad.view(rows, 3 * HEADS, 64), dqkv_r.view(rows, 3 * HEADS, 64), seg, B, ATTN_REL_FLOOR)
    _control(tag + " dqkv/item", per, glob, ATTN_DQKV, 1.5e-2)


# ------------------------------------------------------------------------------------------------------------ 4. encoder layer

# bounds: about 2x the worst of both runs on an MI355X (measured worst / largest median)
ENC_Y_ROW = 8e-3         # output per row, relative L2 (4.2e-3 / 3.3e-3; 2x is 8.4e-3, capped at the stack test's global 8e-3)
ENC_DX_ROW = 9e-3        # dx per row (4.4e-3 / 3.4e-3; stack test 2.5e-2)
ENC_W_ROW = 1.5e-2       # weight gradients per output row, relative L2 (7.1e-3 / 4.9e-3; stack test 4e-2)
ENC_VEC = 4e-2           # bias / LayerNorm gradients per element / rms (2.2e-2 / 3.3e-3; 2x is 4.3e-2, capped at the stack test's 4e-2)


def _site(seed, k, thresh16):
    """the layer's dropout sites (layer.hip site_drop): 0 attention probabilities, 1 attention output, 2 FFN output"""
    from mvp_pytorch_amd import hip
    d = hip.Dropout()
    d.seed_lo = ((seed & 0xFFFFFFFF) ^ ((0x9E3779B9 * (k + 1)) & 0xFFFFFFFF)) & 0xFFFFFFFF
    d.seed_hi = ((seed >> 32) + 0x85EBCA6B * (k + 1)) & 0xFFFFFFFF
    d.thresh16, d.pad_ = thresh16, 0
    return d


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_encoder_layer_joint_size_against_float64_oracle(dev, p_drop):
    """One BERT-base CaptionBertEncoder layer (forward_rows, row-packed) on the joint stack's 37 748 rows in ~515 sequences of
    20 - 125 rows, against oracle.encoder_layer in float64 on the padded layout with bf16-rounded weights.  p_drop = 0.1:
    the three dropout sites' masks replayed (element index m * H + n of the packed rows; ((seq * heads + h) * Lmax + q) * Lp
    + key for the probabilities) and the row count on the device (rows_dev) inside a 44 000-row bound.  Per row of the
    output, per row of dx, per output row of every weight gradient and per element of every vector gradient
    (attention.self.key.bias is exempt: its true gradient is zero, softmax is invariant to it).
    Measured on an MI355X (worst / median, worse of the two runs): y 4.2e-3 / 3.3e-3 and dx 4.4e-3 / 3.4e-3 per row, weight
    gradients 7.1e-3 / 4.9e-3 per output row (attention.output.dense), vector gradients 2.2e-2 / 3.3e-3 per element / rms
    (intermediate.dense.bias); bounds ENC_* above.
    Negative controls: dx of one row (the last of sequence 0) taken from its neighbour: 1.4 on that row (>= 150x ENC_DX_ROW),
    global 7.1e-3 under the stack test's 2.5e-2; one row of intermediate.dense.weight's gradient taken from its neighbour:
    1.5 (>= 95x ENC_W_ROW), global 2.4e-2 under the stack test's 4e-2."""
    from mvp_pytorch_amd import engine, modeling
    _zero_salt(dev)
    H, heads, rows, bound = 768, 12, 37748, 44000
    cfg = dict(gu.BASE_CFG, num_hidden_layers=1, hidden_dropout_prob=p_drop, attention_probs_dropout_prob=p_drop)
    torch.manual_seed(0)
    enc = modeling.modeling_vlbert.CaptionBertEncoder(modeling.make_config(cfg)).to(dev).train()
    g = torch.Generator().manual_seed(37748)
    lens = torch.randint(20, 126, (600,), generator=g)
    B = int((torch.cumsum(lens, 0) <= rows).sum())
    lens = lens[:B].clone()
    short = torch.argsort(lens)[: rows - int(lens.sum())]
    lens[short] += 1                                            # exactly `rows` rows, still 20 - 125 each
    assert int(lens.sum()) == rows and int(lens.max()) <= 125
    lmax = int(lens.max())
    x = _bf(torch.randn(rows, H, generator=g) * 0.5).to(dev)
    dy = _bf(torch.randn(rows, H, generator=g) * 0.1).to(dev)
    lens_d = lens.to(torch.int32).to(dev)
    starts = (torch.cumsum(lens_d, 0) - lens_d).to(torch.int32)
    seed = 0x0DDB_A11_5EED_0001
    orig = engine.next_seed
    engine.next_seed = lambda: seed
    try:
        if p_drop > 0:
            xin = torch.zeros(bound, H, dtype=torch.bfloat16, device=dev)
            xin[:rows] = x
            xin.requires_grad_(True)
            cnt = torch.tensor([rows, lmax], dtype=torch.int64, device=dev)
            y = enc.forward_rows(xin, starts, lens_d, B, lmax, rows_dev=cnt)
            dyb = torch.zeros(bound, H, dtype=torch.bfloat16, device=dev)
            dyb[:rows] = dy
            y.backward(dyb)
            y, dx = y[:rows], xin.grad[:rows]
        else:
            xin = x.clone().requires_grad_(True)
            y = enc.forward_rows(xin, starts, lens_d, B, lmax)
            y.backward(dy)
            dx = xin.grad
        torch.cuda.synchronize()
    finally:
        engine.next_seed = orig

    seg = torch.repeat_interleave(torch.arange(B, device=dev), lens.to(dev))
    pad_idx = seg * lmax + (torch.arange(rows, device=dev) - starts.long()[seg])
    drops = None
    if p_drop > 0:
        from mvp_pytorch_amd import hip
        t16 = int(round(p_drop * 65536.0))
        sc = 65536.0 / (65536.0 - t16)
        Lp = (lmax + 31) // 32 * 32
        attn = hip.dropout_mask(_site(seed, 0, t16), B * heads * lmax * Lp, dev).view(B, heads, lmax, Lp)[..., :lmax].to(F64)
        dense = []
        for k in (1, 2):
            kp = torch.ones(B * lmax, H, dtype=F64, device=dev)
            kp[pad_idx] = hip.dropout_mask(_site(seed, k, t16), rows * H, dev).view(rows, H).to(F64)
            dense.append(kp.view(B, lmax, H))
        drops = {"attn": (attn, sc), "attn_out": (dense[0], sc), "ffn_out": (dense[1], sc)}
    sd = {"enc." + k: (v.detach().to(torch.bfloat16) if v.dim() == 2 else v.detach()).to(F64).requires_grad_(True)
          for k, v in enc.state_dict().items()}
    xp = torch.zeros(B * lmax, H, dtype=F64, device=dev)
    xp[pad_idx] = x.to(F64)
    xp = xp.view(B, lmax, H).requires_grad_(True)
    valid = torch.zeros(B * lmax, dtype=torch.long, device=dev)
    valid[pad_idx] = 1
    yo = orc.encoder_layer(sd, "enc.layer.0", xp, orc.extended_mask(valid.view(B, lmax), F64), heads, cfg["layer_norm_eps"],
                           drops)
    dyp = torch.zeros(B * lmax, H, dtype=F64, device=dev)
    dyp[pad_idx] = dy.to(F64)
    yo.backward(dyp.view(B, lmax, H))
    y_r, dx_r = yo.detach().view(-1, H)[pad_idx], xp.grad.view(-1, H)[pad_idx]
    tag = "enc p=%.1f" % p_drop
    print("%s: %d sequences, %d rows, Lmax %d" % (tag, B, rows, lmax))
    _check(tag + " y/row", *_unit_rel(y.view(rows, 1, H), y_r.view(rows, 1, H)), ENC_Y_ROW)
    _check(tag + " dx/row", *_unit_rel(dx.view(rows, 1, H), dx_r.view(rows, 1, H)), ENC_DX_ROW)
    names = [n for n, _ in enc.named_parameters()]
    assert len(names) == 16
    for n, p in enc.named_parameters():
        if n.endswith("attention.self.key.bias"):
            continue
        want = sd["enc." + n].grad
        if p.dim() == 2:
            _check(tag + " " + n, *_unit_rel(p.grad.unsqueeze(1), want.unsqueeze(1)), ENC_W_ROW)
        else:
            _check(tag + " " + n, *_col_rel(p.grad, want), ENC_VEC)
    # negative controls
    r0 = int(lens[0]) - 1
    dx_bad = dx_r.clone()
    dx_bad[r0] = dx_r[r0 - 1]
    _control(tag + " dx/row", *_unit_rel(dx_bad.view(rows, 1, H), dx_r.view(rows, 1, H)), ENC_DX_ROW, 2.5e-2)
    w = sd["enc.layer.0.intermediate.dense.weight"].grad
    w_bad = w.clone()
    w_bad[-1] = w[-2]
    _control(tag + " W_i row", *_unit_rel(w_bad.unsqueeze(1), w.unsqueeze(1)), ENC_W_ROW, 4e-2)
