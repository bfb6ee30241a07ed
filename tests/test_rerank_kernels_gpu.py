"""ste_xattn_mq_fwd and ste_xattn_gather_fwd (csrc/xattn_mq.hip) against float64.

xattn_mq_fwd: the reference is float64 attention on the CPU from the same fp32 q and the widened
bf16 K/V, masked keys at -1e9.  With |q|, |k| <= 1 the bound is elementwise

    |out - ref| <= 2^-8 · Σ_s p_s·|v_s,c|        (p the float64 softmax)

which is derived, not measured: the probabilities are rounded once to bf16 for P·V (2^-9 relative
per term), the hi + lo query split and the fp32 accumulation stay below 2^-12 at these magnitudes,
so the bound is twice the rounding unit.  Every case prints its worst ratio to the bound; measured
on an MI355X the worst is 2.57e-3 (P = 1024, S = 31) against 3.91e-3, and 1.9e-4 at S = 1500.

Shapes: head dims 8, 24 (padded to 32 for Q·Kᵀ and 16 / 32 output columns), 16, 96 (3 of 4 d steps
of the 128 instantiation), 256 (two staged column halves of V); S = 1, 5, 31, 32, 33 around one
32-key tile, 129 = 5 tiles (wave 0 takes two, the others one), 1500 = 47 tiles (12 per wave, one
wave 11); C = 1, 15, 16, 17, 40 around the 16-query tile; B = 1, 3; no mask, a ragged mask and a
fully masked clip; empty (-1) and repeated slots; ldkv = 2P (the engine's K|V view) and 2P + 8.

xattn_gather_fwd must equal ops.xattn1_fwd(drop_p=0) on the replicated operands bitwise.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -8


@pytest.fixture(scope="module")
def ops():
    from speech_transcript_embeddings_amd import ops as o
    return o


def _kv(B, S, P, pad, g):
    """bf16 K|V buffer [B*S, 2P + pad] and its two column views (|k| <= 1)."""
    buf = torch.zeros(B * S, 2 * P + pad, dtype=torch.bfloat16)
    buf[:, :P] = (torch.rand(B * S, P, generator=g) * 2 - 1).to(torch.bfloat16)
    buf[:, P:2 * P] = torch.randn(B * S, P, generator=g).to(torch.bfloat16)
    return buf


def _mask(kind, B, S, g):
    if kind == "none":
        return None
    m = torch.ones(B, S, dtype=torch.int32)
    for b in range(B):
        m[b, int(torch.randint(1, S + 1, (1,), generator=g)):] = 0   # ragged: 1..S valid keys
    if kind == "full":
        m[B - 1] = 0                                                  # one clip with no valid key
    return m.reshape(-1)


def _ref(q, rows, k, v, mask, S, nh):
    """float64 attention of query rows `rows` [R] over K/V block blk[r]: (out, Σ p|v|) [R, P]."""
    qrow, blk = rows
    R, P = len(qrow), q.shape[1]
    d = P // nh
    out = torch.zeros(R, P, dtype=torch.float64)
    bound = torch.zeros(R, P, dtype=torch.float64)
    k, v, q = k.double(), v.double(), q.double()
    for r in range(R):
        if qrow[r] < 0 or blk[r] < 0:
            continue
        kb = k[blk[r] * S:(blk[r] + 1) * S].reshape(S, nh, d)
        vb = v[blk[r] * S:(blk[r] + 1) * S].reshape(S, nh, d)
        a = torch.einsum("hd,shd->hs", q[qrow[r]].reshape(nh, d), kb) * d ** -0.5
        if mask is not None:
            a = a.masked_fill(mask[blk[r] * S:(blk[r] + 1) * S].view(1, S) == 0, -1e9)
        p = a.softmax(-1)
        out[r] = torch.einsum("hs,shd->hd", p, vb).reshape(P)
        bound[r] = torch.einsum("hs,shd->hd", p, vb.abs()).reshape(P)
    return out, bound


def _qrow(kind, B, C, U, g):
    qrow = torch.randint(0, U, (B * C,), generator=g, dtype=torch.int32)
    if kind == "empty":
        qrow[torch.rand(B * C, generator=g) < 0.3] = -1
        qrow[0] = -1
    elif kind == "repeat":
        qrow[:] = qrow[0]
        qrow[B * C // 2:] = (qrow[0] + 1) % U
    return qrow


# (P, nh, B, C, S, mask, ldkv pad, qrow)
MQ_CASES = [
    (32, 4, 1, 1, 1, "none", 0, "plain"),
    (32, 4, 3, 15, 5, "ragged", 8, "empty"),
    (32, 4, 1, 40, 33, "full", 0, "repeat"),
    (96, 4, 3, 16, 31, "ragged", 0, "plain"),
    (96, 4, 1, 17, 129, "none", 8, "empty"),
    (96, 4, 3, 1, 32, "full", 0, "plain"),
    (128, 8, 3, 40, 129, "ragged", 0, "empty"),
    (128, 8, 1, 16, 32, "none", 8, "repeat"),
    (128, 8, 3, 17, 33, "full", 0, "plain"),
    (128, 8, 1, 3, 1500, "ragged", 0, "plain"),
    (768, 8, 3, 17, 33, "ragged", 8, "empty"),
    (768, 8, 1, 15, 129, "none", 0, "plain"),
    (768, 8, 3, 1, 5, "full", 0, "repeat"),
    (1024, 4, 1, 16, 31, "ragged", 0, "plain"),
    (1024, 4, 3, 40, 129, "full", 8, "empty"),
    (1024, 4, 1, 1, 1, "none", 0, "plain"),
]


@pytest.mark.parametrize("P,nh,B,C,S,mask_kind,pad,qkind", MQ_CASES)
def test_xattn_mq_fwd(ops, P, nh, B, C, S, mask_kind, pad, qkind):
    g = torch.Generator().manual_seed(P * 31 + S * 7 + C)
    U = 11
    q = torch.rand(U, P, generator=g) * 2 - 1
    kv = _kv(B, S, P, pad, g)
    mask = _mask(mask_kind, B, S, g)
    qrow = _qrow(qkind, B, C, U, g)
    dev = "cuda"
    kvd = kv.to(dev)
    out = torch.full((B * C, P), float("nan"), device=dev)
    ops.xattn_mq_fwd(q.to(dev), qrow.to(dev), kvd[:, :P], kvd[:, P:2 * P], None if mask is None else mask.to(dev),
                     B, C, S, nh, out)
    torch.cuda.synchronize()
    out = out.cpu().double()
    blk = torch.arange(B).repeat_interleave(C).tolist()
    ref, bound = _ref(q, (qrow.tolist(), blk), kv[:, :P], kv[:, P:2 * P], mask, S, nh)
    empty = qrow < 0
    assert torch.equal(out[empty], torch.zeros_like(out[empty])), "an empty slot's row is exactly zero"
    assert torch.isfinite(out).all()
    live = ~empty
    ratio = ((out - ref).abs()[live] / bound[live].clamp_min(1e-300)).max().item() if live.any() else 0.0
    print(f"xattn_mq P={P} nh={nh} B={B} C={C} S={S} {mask_kind}/{qkind}: max |err| / Σp|v| = {ratio:.3e} "
          f"(bound {BOUND:.3e})")
    assert ((out - ref).abs() <= BOUND * bound)[live].all(), ratio


def test_xattn_mq_invariance(ops):
    """A slot's row is bit-identical inside C = 40 among other queries, alone (C = 1, B = 1) and at
    another slot of another batch among different neighbours."""
    P, nh, S, B, C, U = 128, 8, 129, 3, 40, 50
    g = torch.Generator().manual_seed(5)
    dev = "cuda"
    q = (torch.rand(U, P, generator=g) * 2 - 1).to(dev)
    kv = _kv(B, S, P, 0, g).to(dev)
    mask = _mask("ragged", B, S, g).to(dev)
    qrow = torch.randint(0, U, (B * C,), generator=g, dtype=torch.int32).to(dev)
    big = torch.empty(B * C, P, device=dev)
    ops.xattn_mq_fwd(q, qrow, kv[:, :P], kv[:, P:], mask, B, C, S, nh, big)
    for b, c in ((1, 23), (0, 0), (2, 39)):
        row = qrow[b * C + c:b * C + c + 1].clone()
        clip = kv[b * S:(b + 1) * S]
        alone = torch.empty(1, P, device=dev)
        ops.xattn_mq_fwd(q, row, clip[:, :P], clip[:, P:], mask[b * S:(b + 1) * S].contiguous(), 1, 1, S, nh, alone)
        assert torch.equal(alone[0], big[b * C + c]), (b, c)
        # the same clip as the second of two, the query at slot 5 of 17 among other queries
        C2 = 17
        kv2 = torch.cat([kv[((b + 1) % B) * S:((b + 1) % B + 1) * S], clip]).contiguous()
        m2 = torch.cat([mask[((b + 1) % B) * S:((b + 1) % B + 1) * S], mask[b * S:(b + 1) * S]]).contiguous()
        qrow2 = torch.randint(0, U, (2 * C2,), generator=g, dtype=torch.int32).to(dev)
        qrow2[C2 + 5] = row[0]
        other = torch.empty(2 * C2, P, device=dev)
        ops.xattn_mq_fwd(q, qrow2, kv2[:, :P], kv2[:, P:], m2, 2, C2, S, nh, other)
        assert torch.equal(other[C2 + 5], big[b * C + c]), (b, c)


# (P, nh, R, S)
GATHER_CASES = [(32, 4, 1, 1), (32, 4, 70, 257), (96, 4, 7, 12), (96, 4, 70, 64), (128, 8, 70, 12), (128, 8, 7, 257),
                (768, 8, 7, 64), (768, 8, 1, 12), (1024, 4, 7, 257), (1024, 4, 70, 1)]


@pytest.mark.parametrize("P,nh,R,S", GATHER_CASES)
def test_xattn_gather_fwd(ops, P, nh, R, S):
    """Bitwise ops.xattn1_fwd(drop_p=0) on the replicated queries, keys, values and masks; repeated
    qrow and kvblk entries, ragged masks, -1 pairs exactly zero; K and V are views of a padded buffer."""
    g = torch.Generator().manual_seed(P + R * 13 + S)
    dev = "cuda"
    NQ, NB = 5, 6
    q = (torch.rand(NQ, P, generator=g) * 2 - 1).to(dev)
    kv = _kv(NB, S, P, 8, g).to(dev)
    mask = _mask("ragged", NB, S, g).to(dev)
    qrow = torch.randint(0, NQ, (R,), generator=g, dtype=torch.int32)
    kvblk = torch.randint(0, NB, (R,), generator=g, dtype=torch.int32)
    if R > 1:
        qrow[1], kvblk[1] = qrow[0], kvblk[0]       # a repeated pair
        kvblk[R - 1] = -1                            # an empty pair
    if R > 8:
        kvblk[3::9] = -1
        kvblk[4], kvblk[5] = 2, 2                    # a repeated block with different queries
    out = torch.full((R, P), float("nan"), device=dev)
    ops.xattn_gather_fwd(q, qrow.to(dev), kv[:, :P], kv[:, P:2 * P], kvblk.to(dev), mask, R, S, nh, out)
    # replicated operands for the existing single-query kernel
    blk = kvblk.clamp(min=0).long()
    rows = (blk.view(R, 1) * S + torch.arange(S).view(1, S)).reshape(-1).to(dev)
    kvrep = kv.index_select(0, rows).contiguous()
    ref = torch.empty(R, P, device=dev)
    ops.xattn1_fwd(q.index_select(0, qrow.long().to(dev)).contiguous(), kvrep[:, :P], kvrep[:, P:2 * P],
                   mask.index_select(0, rows).contiguous(), R, S, nh, torch.empty(R * nh * S, device=dev), ref, drop_p=0.0)
    ref[(kvblk < 0).to(dev)] = 0.0
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert torch.equal(out[(kvblk < 0).to(dev)], torch.zeros(int((kvblk < 0).sum()), P, device=dev))
