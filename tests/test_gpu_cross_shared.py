"""The shared-logit form of LightGlue's cross blocks alone (rfe_k_cross_attention, form = 1) against a float64 softmax attention per pair, head and
direction.  The cross blocks share one projection for queries and keys, so both directions of a pair attend through the same matrix S = qk0 . qk1^T:
lg_attention_dma_kernel<true> runs side 0 and writes its logits out, lg_cross_slog_kernel runs side 1 from them (lg_kernels.hip).  The shapes are the
smallest at which the form can go wrong: L no multiple of the 32-key tile (partial tiles in both directions, non-square live blocks), an odd pair
count (padded (pair, head) units), empty sides, more than one query block on one side and less than one key tile on the other.  The workspace is the
library's own, so the HOOK fills all of it -- the logit scratch included -- with NaN before every call, the second call of a case too, and the test
fills the output with NaN: a stale or unwritten logit, or an output word the kernels skip, shows as a non-finite result.
The generic form (form = 2) meets the same bound on the same input.  Bound: tests/test_gpu_attention.py's, 2e-5 on O(1) values."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ATT_TOL = 2e-5   # max |context - float64| for O(1) values (tests/test_gpu_attention.py)

CASES = {
    # name: (P, L, lengths of (side 0, side 1) per pair, lengths of the second call on the same context)
    "ragged_L100": (3, 100, [(100, 100), (100, 37), (33, 100)], [(37, 100), (64, 64), (100, 5)]),
    "empty_sides_L64": (3, 64, [(64, 64), (0, 50), (50, 0)], [(50, 33), (64, 64), (0, 64)]),
    "blocks_L160": (1, 160, [(129, 31)], [(31, 129)]),
}


@pytest.fixture(scope="module")
def ctx():
    from rover_slam_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _attention_f64(q, k, v, nq, nk):
    """q [L,256], k / v [L,256] float32 -> context [L,256] float64; rows >= nq are zero, and every row when there is no key."""
    qq, kk, vv = q.astype(np.float64)[:nq], k.astype(np.float64)[:nk], v.astype(np.float64)[:nk]
    out = np.zeros((q.shape[0], 256))
    if nk == 0:
        return out
    for h in range(4):
        s = qq[:, 64 * h:64 * h + 64] @ kk[:, 64 * h:64 * h + 64].T * 0.125
        s -= s.max(1, keepdims=True)
        p = np.exp(s)
        p /= p.sum(1, keepdims=True)
        out[:nq, 64 * h:64 * h + 64] = p @ vv[:, 64 * h:64 * h + 64]
    return out


@pytest.fixture(scope="module")
def inputs():
    """per case: the [qk | v] rows (shared by every test of the case, never modified)"""
    data = {}
    for name, (P, L, _, _) in CASES.items():
        rng = np.random.default_rng(P * 1000 + L)
        x = rng.standard_normal((2 * P * L, 512)).astype(np.float32)
        x[:, :256] *= 1.5                                    # logits with a standard deviation of ~2.3, peaky rows
        x[::7, 3] += 6.0                                     # dominant keys / queries planted late: the softmax reference moves after the first tile,
        x[L // 2::11, 5] += 9.0                              # in both directions (the rows are queries of one direction and keys of the other)
        data[name] = x
    return data


def _reference(x, P, L, lens):
    xs = x.reshape(2 * P, L, 512)
    ref = np.zeros((2 * P, L, 256))
    for p in range(P):
        n0, n1 = lens[p]
        ref[p] = _attention_f64(xs[p][:, :256], xs[p + P][:, :256], xs[p + P][:, 256:], n0, n1)
        ref[p + P] = _attention_f64(xs[p + P][:, :256], xs[p][:, :256], xs[p][:, 256:], n1, n0)
    return ref


def _run(ctx, capi, dx, dout, P, L, lens, form):
    flat = np.array([a for a, _ in lens] + [b for _, b in lens], np.int32)   # side-major: all side-0 lengths, then all side-1
    dlen = ctx.alloc(flat.nbytes)
    dlen.upload(flat)
    dout.upload(np.full((2 * P * L, 256), np.nan, np.float32))
    ctx._chk(capi.lib.rfe_k_cross_attention(ctx.h, dx.ptr, 512, dout.ptr, P, L, dlen.ptr, form))
    out = dout.download((2 * P, L, 256), np.float32)
    dlen.free()
    return out, flat


@pytest.mark.parametrize("name", list(CASES))
def test_cross_shared_logits_vs_float64(ctx, inputs, name):
    from rover_slam_amd import capi
    P, L, lens_a, lens_b = CASES[name]
    x = inputs[name]
    dx = ctx.alloc(x.nbytes)
    dx.upload(x)
    dout = ctx.alloc(2 * P * L * 1024)
    try:
        # the second call runs on the same context (and so the same logit scratch) with other lengths: it must not see the first call's logits
        for lens in (lens_a, lens_b):
            ref = _reference(x, P, L, lens)
            for form in (1, 2):
                out, flat = _run(ctx, capi, dx, dout, P, L, lens, form)
                assert np.isfinite(out).all(), (name, lens, form)
                for s in range(2 * P):
                    assert not out[s][flat[s]:].any(), "context rows past the sequence length must be zero"
                    if flat[(s + P) % (2 * P)] == 0:
                        assert not out[s].any(), "a side with no keys to attend to must come out zero"
                err = float(np.abs(out - ref).max())
                print(f"cross attention {name} lens={lens} form={form}: max |context - float64| {err:.2e}")
                assert err < ATT_TOL, (name, lens, form, err)
    finally:
        dx.free()
        dout.free()
