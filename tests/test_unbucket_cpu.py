"""``effort_amd.weights.unbucket`` on the host: the specification of the matrix ``Decoder.prefill(weights="buckets")`` multiplies by.

The buckets come from the CPU converter the other CPU tests use (oracle/cpu.py).  Its whole-matrix call takes outDim 32 (4096 % outDim
== 0); 96 and 1056 are bucketized input row by input row with ``bucketize_row``, which is that call's inner step (checked below on the
shape both take).  The matrices hold no zero: a real zero ties with the zero padding of a non-power-of-two row and sends the row down
the literal preBucketize path, whose bundles are the ones ``unbucket`` may refuse."""
import numpy as np
import pytest
import torch

IN_DIM = 4096
OUT_DIMS = (32, 96, 1056)
NAN16 = 0x7E00


def matrix(outDim, inDim=IN_DIM, seed=0):
    rng = np.random.default_rng([seed, outDim, inDim])
    W = (rng.standard_normal((outDim, inDim), dtype=np.float32) * np.float32(0.02)).astype(np.float16)
    u = W.view(np.uint16)
    u[(u & 0x7FFF) == 0] = 0x0400                            # no zero (see the module's docstring)
    return W


_BUCKETS = {}


def bucketized(outDim):
    """(W f16 [outDim, IN_DIM], buckets u16 [16 * IN_DIM, outDim / 16]), computed once per shape and left unchanged."""
    if outDim not in _BUCKETS:
        from oracle import cpu
        W = matrix(outDim)
        b = np.zeros((16, IN_DIM, outDim // 16), np.uint16)
        for j in range(IN_DIM):
            ranked, dropped = cpu.bucketize_row(W[:, j], 16)
            assert dropped == 0
            b[:, j, :] = ranked.view(np.uint16)
        _BUCKETS[outDim] = (W, b.reshape(16 * IN_DIM, outDim // 16))
    return _BUCKETS[outDim]


def u16(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def check_is_w_with_positions(U, W):
    Uu, Wu = u16(U), W.view(np.uint16)
    assert Uu.shape == (1,) + Wu.shape and U.dtype == torch.float16
    assert ((Uu[0] & 0xFFF0) == (Wu & 0xFFF0)).all()
    assert ((Uu[0] & 15) == (np.arange(Wu.shape[0])[:, None] % 16)).all()


def test_row_by_row_is_the_converter():
    from oracle import cpu
    W, b = bucketized(32)
    whole, _, _, dropped = cpu.convert_fp16(W)
    assert dropped == 0 and (whole.view(np.uint16) == b).all()


@pytest.mark.parametrize("outDim", OUT_DIMS)
def test_unbucket_gives_the_matrix_with_positions(outDim):
    from effort_amd.weights import unbucket
    W, b = bucketized(outDim)
    check_is_w_with_positions(unbucket(torch.from_numpy(b.view(np.int16)), IN_DIM, outDim), W)
    check_is_w_with_positions(unbucket(torch.from_numpy(b.view(np.float16)), IN_DIM, outDim), W)      # f16 words, one expert's 2-d tensor


@pytest.mark.parametrize("outDim", OUT_DIMS)
def test_unbucket_ignores_the_pitch_padding(outDim):
    from effort_amd.weights import unbucket
    W, b = bucketized(outDim)
    cols = outDim // 16
    pitch = (cols * 2 + 127) // 128 * 64 + 64                # words: whole 128-byte lines and one more
    store = np.full((1, 16 * IN_DIM, pitch), NAN16, np.uint16)
    store[0, :, :cols] = b
    view = torch.from_numpy(store.view(np.int16))[:, :, :cols]
    assert not view.is_contiguous()
    check_is_w_with_positions(unbucket(view, IN_DIM, outDim), W)
    check_is_w_with_positions(unbucket(torch.from_numpy(store.view(np.int16)), IN_DIM, outDim), W)   # the whole pitched tensor: columns past the payload are not read


def test_unbucket_of_a_stack():
    from effort_amd.weights import unbucket
    W, b = bucketized(96)
    other = np.roll(b, 1, axis=0).copy()                      # another valid layout: input j of every rank moved to j + 1
    U = unbucket(torch.from_numpy(np.stack([b, other]).view(np.int16)), IN_DIM, 96)
    assert tuple(U.shape) == (2, 96, IN_DIM)
    assert (u16(U)[1][:, 1:] == u16(U)[0][:, :-1]).all()


def test_a_duplicate_position_raises():
    from effort_amd.weights import unbucket
    _, b = bucketized(96)
    b = b.copy()
    j, c = 1234, 3
    b[5 * IN_DIM + j, c] = (b[5 * IN_DIM + j, c] & 0xFFF0) | (b[9 * IN_DIM + j, c] & 15)      # rank 5 names rank 9's output
    with pytest.raises(ValueError, match="same output position"):
        unbucket(torch.from_numpy(b.view(np.int16)), IN_DIM, 96)


def test_a_zero_entry_is_skipped():
    from effort_amd.weights import unbucket
    W, b = bucketized(96)
    b = b.copy()
    j, c, r = 77, 2, 11
    pos = int(b[r * IN_DIM + j, c] & 15)
    b[r * IN_DIM + j, c] = 0
    U = u16(unbucket(torch.from_numpy(b.view(np.int16)), IN_DIM, 96))[0]
    assert U[16 * c + pos, j] == 0                            # +0, and nobody else's slot was touched:
    U[16 * c + pos, j] = (W.view(np.uint16)[16 * c + pos, j] & 0xFFF0) | pos
    assert ((U & 0xFFF0) == (W.view(np.uint16) & 0xFFF0)).all() and ((U & 15) == (np.arange(96)[:, None] % 16)).all()


def test_shapes_that_are_not_percent_load_16_raise():
    from effort_amd.weights import unbucket
    _, b = bucketized(32)
    t = torch.from_numpy(b.view(np.int16))
    with pytest.raises(ValueError, match="percentLoad 16"):
        unbucket(t[:8 * IN_DIM], IN_DIM, 32)                  # a truncated bundle
    with pytest.raises(ValueError, match="percentLoad 16"):
        unbucket(t, IN_DIM, 64)                               # fewer columns than the outputs need
    with pytest.raises(ValueError, match="16-bit"):
        unbucket(t.to(torch.int32), IN_DIM, 32)
