"""The sampled pick without a GPU: the Philox generator (Python restatement against published known answers, and the library's own
``effort_sample_bits`` -- the definition the kernel compiles -- against the restatement), the numpy specification ``sample_reference`` on
the edge rows, and the bytes ``Sampling.to_device`` packs."""
import ctypes as C
import struct

import numpy as np
import pytest

from effort_amd.sampling import MAX_K, Sampling, philox4x32_10, philox_bits, philox_bits_many, philox_u, sample_reference, topk_reference


def words(s):
    return tuple(int(w, 16) for w in s.split())


@pytest.mark.parametrize("counter,key,out", [
    ("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, out):
    assert philox4x32_10(words(counter), words(key)) == words(out)


def test_philox_u_is_word_zero_of_the_documented_counter():
    seed, stream, pos = 0x299F31D0A4093822, 0x85A308D3, 0x243F6A88
    x0 = philox4x32_10((pos, stream, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))[0]
    assert philox_bits(seed, stream, pos) == x0
    assert philox_u(seed, stream, pos) == (x0 >> 8) / 2.0 ** 24
    assert 0.0 <= philox_u(seed, stream, pos) < 1.0
    pos_many = np.array([0, 1, 77, 2 ** 32 - 1], dtype=np.uint64)
    assert philox_bits_many(seed, stream, pos_many).tolist() == [philox_bits(seed, stream, int(p)) for p in pos_many]


def test_library_generator_equals_the_python_one(hip_lib_built):
    """effort_sample_bits is the __host__ __device__ function the kernel draws from: 1000 (seed, stream, pos) triples."""
    import effort_amd
    fn = effort_amd.lib().effort_sample_bits
    rng = np.random.default_rng(11)
    cases = [(0, 0, 0), (0, 0, 2 ** 32 - 1), (1 << 63, 0, 0), (0xFFFFFFFF00000000, 7, 5), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1), (12345, 1, 2 ** 31)]
    while len(cases) < 1000:
        cases.append((int(rng.integers(0, 2 ** 64, dtype=np.uint64)), int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32))))
    for seed, stream, pos in cases:
        got = fn(C.c_uint32(seed & 0xFFFFFFFF), C.c_uint32(seed >> 32), C.c_uint32(stream), C.c_uint32(pos))
        assert got == philox_bits(seed, stream, pos), (seed, stream, pos)


def test_uniform_mean():
    """A million draws: the standard deviation of their mean is 0.0003, so 0.002 catches a gross error only."""
    u = (philox_bits_many(2024, 0, np.arange(1_000_000, dtype=np.uint64)) >> 8).astype(np.float64) * 2.0 ** -24
    assert u.min() >= 0.0 and u.max() < 1.0
    assert abs(float(u.mean()) - 0.5) < 0.002


# ---------------------------------------------------------------- sample_reference
def test_top_k_one_is_argmax_with_lowest_index_ties():
    rng = np.random.default_rng(3)
    for trial in range(20):
        x = np.round(rng.standard_normal(300) * 2).astype(np.float32)            # many ties, the maximum among them
        want = int(np.argmax(x))                                                # numpy: first occurrence
        assert sample_reference(x, Sampling(top_k=1, temperature=1.3, seed=trial), pos=trial) == (want, np.inf)
        assert sample_reference(x, Sampling(top_k=40, temperature=0.0, seed=trial), pos=trial)[0] == want
        assert sample_reference(x, Sampling(top_k=40, temperature=float("nan")), pos=trial)[0] == want
        assert sample_reference(x, Sampling(top_k=40, temperature=float("inf")), pos=trial)[0] == want


def test_top_p_to_zero_keeps_one_entry():
    rng = np.random.default_rng(4)
    x = rng.standard_normal(1000).astype(np.float32)
    for pos in range(200):
        assert sample_reference(x, Sampling(top_k=64, top_p=1e-9, temperature=5.0, seed=9), pos)[0] == int(np.argmax(x))
    # ... and a top_p outside (0, 1] counts as 1: the draws spread
    assert len({sample_reference(x, Sampling(top_k=64, top_p=0.0, temperature=5.0, seed=9), pos)[0] for pos in range(200)}) > 20
    assert [sample_reference(x, Sampling(top_k=64, top_p=7.0, temperature=5.0, seed=9), pos) for pos in range(50)] == \
           [sample_reference(x, Sampling(top_k=64, top_p=1.0, temperature=5.0, seed=9), pos) for pos in range(50)]


def test_two_token_distribution_is_three_to_one():
    """Weights 3 : 1 -- logits log 3 and 0 at temperature 1, top_k 2 -- over pos = 0 .. 19999: the first token's share is 0.75 within
    0.012, four standard deviations (sqrt(0.75 * 0.25 / 20000) = 0.0031)."""
    x = np.full(50, -30.0, dtype=np.float32)
    x[17], x[4] = np.log(3.0), 0.0
    s = Sampling(temperature=1.0, top_k=2, seed=31337)
    picks = [sample_reference(x, s, pos)[0] for pos in range(20000)]
    assert set(picks) == {17, 4}
    assert abs(picks.count(17) / 20000 - 0.75) <= 0.012


def test_margin_is_the_distance_to_the_nearest_boundary():
    x = np.array([0.0, 0.0, 0.0, 0.0], dtype=np.float32)                         # four equal weights: boundaries at 1/4, 2/4, 3/4, 1
    s = Sampling(temperature=1.0, top_k=4, seed=5)
    for pos in range(100):
        u = philox_u(5, 0, pos)
        pick, margin = sample_reference(x, s, pos)
        assert pick == int(u * 4)
        assert abs(margin - min(abs(u - b) for b in (0.25, 0.5, 0.75, 1.0))) < 1e-12


def test_edge_rows():
    nan, inf = float("nan"), float("inf")
    s = Sampling(temperature=1.0, top_k=8, seed=2)
    # every logit NaN: token 0
    assert sample_reference(np.full(9, nan, dtype=np.float32), s, 0) == (0, np.inf)
    # NaN is never selected; -inf is an ordinary smallest value with weight 0
    x = np.array([nan, -inf, 1.0, nan, -inf, 1.0], dtype=np.float32)
    idx, val = topk_reference(x, 8)
    assert idx.tolist() == [2, 5, 1, 4] and val.tolist() == [1.0, 1.0, -inf, -inf]
    assert {sample_reference(x, s, pos)[0] for pos in range(100)} == {2, 5}
    # all equal: the result is indices 0 .. K-1, and every one of them is drawn
    x = np.full(100, 2.5, dtype=np.float32)
    assert topk_reference(x, 8)[0].tolist() == list(range(8))
    assert {sample_reference(x, s, pos)[0] for pos in range(400)} == set(range(8))
    # the two zeros tie: index order decides, the values come back as stored
    x = np.array([-1.0, -0.0, 0.0, -0.0, 0.0], dtype=np.float32)
    idx, val = topk_reference(x, 3)
    assert idx.tolist() == [1, 2, 3] and np.signbit(val).tolist() == [True, False, True]
    # all -inf, and +inf on top: rank 0
    assert sample_reference(np.full(5, -inf, dtype=np.float32), s, 3) == (0, np.inf)
    assert sample_reference(np.array([0.0, inf, 3.0, inf], dtype=np.float32), s, 3) == (1, np.inf)
    # n < K: K becomes n
    assert {sample_reference(np.array([0.0, 0.1], dtype=np.float32), Sampling(top_k=64, seed=1), pos)[0] for pos in range(64)} == {0, 1}


def test_host_side_validation():
    for bad in (0, 65, -1, 2.5):
        with pytest.raises(ValueError):
            Sampling(top_k=bad)
    assert Sampling(top_k=1).top_k == 1 and Sampling(top_k=MAX_K).top_k == 64
    with pytest.raises(ValueError):
        Sampling(seed=-1)
    with pytest.raises(ValueError):
        Sampling(stream=1 << 32)


def test_to_device_packs_the_documented_bytes():
    import torch
    s = Sampling(temperature=0.7, top_k=40, top_p=0.9, seed=0x0123456789ABCDEF, stream=3)
    t = s.to_device()
    assert t.dtype == torch.uint8 and t.numel() == 32
    raw = bytes(t.tolist())
    assert raw == struct.pack("<f", 0.7) + struct.pack("<f", 0.9) + struct.pack("<6I", 40, 0x89ABCDEF, 0x01234567, 3, 0, 0)
    target = torch.zeros(32, dtype=torch.uint8)
    assert Sampling(top_k=1, seed=1 << 32).to_device(target) is target
    assert struct.unpack("<ffIIIIII", bytes(target.tolist())) == (1.0, 1.0, 1, 0, 1, 0, 0, 0)
    with pytest.raises(ValueError):
        s.to_device(torch.zeros(16, dtype=torch.uint8))


def test_struct_layout_in_the_header():
    """The header's struct is what ``pack`` writes: 32 bytes, the documented field order (compiled as C11 with offsetof)."""
    import os
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = ('#include <stddef.h>\n#include "effort_hip.h"\n'
           '_Static_assert(sizeof(effort_sample_params) == 32, "size");\n'
           '_Static_assert(offsetof(effort_sample_params, temperature) == 0 && offsetof(effort_sample_params, top_p) == 4 && '
           'offsetof(effort_sample_params, top_k) == 8 && offsetof(effort_sample_params, seed_lo) == 12 && '
           'offsetof(effort_sample_params, seed_hi) == 16 && offsetof(effort_sample_params, stream) == 20 && '
           'offsetof(effort_sample_params, reserved) == 24, "layout");\n_Static_assert(EFFORT_SAMPLE_MAX_K == 64, "max k");\n')
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "layout.c")
        with open(path, "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(root, "include"), path])
