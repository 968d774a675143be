"""The device ray loader's host side (no GPU): the epoch permutation and the sun-check rays through the C ABI's host mirrors (which share their integer
arithmetic with the kernels, csrc/loader_common.h), the generator's known-answer vectors, the argument errors of snerf_loader_create (raised before
anything touches a GPU) and the Python mirror of the epoch layout.

The statistical bounds are conditions set in advance, not measurements: for a uniformly random permutation of N = 100003 elements the expected number
of agreements between two independent permutations, of fixed points and of adjacent neighbours is 1, 1 and 2 (Poisson: P(> 10) < 1e-8, P(> 12 | mean 2)
< 1e-6), and corr(i, p[i]) has standard deviation 1 / sqrt(N - 1) = 0.0032."""
import ctypes as C

import numpy as np
import pytest

SIZES = [1, 2, 3, 5, 96, 1000, 4095, 4096, 4097, 100003]
N_BIG = 100003


@pytest.fixture(scope="module")
def L():
    from season_nerf_amd import loader
    return loader


@pytest.fixture(scope="module")
def big(L):
    """The permutations of N = 100003 the statistical tests share: (seed 0, epoch 0), (seed 0, epoch 1), (seed 1, epoch 0)."""
    out = {(s, e): L.host_indices(N_BIG, s, e) for s, e in ((0, 0), (0, 1), (1, 0))}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_indices_are_a_permutation(L, n):
    for seed, epoch in ((0, 0), (7, 3)):
        p = L.host_indices(n, seed, epoch)
        assert p.dtype == np.int64 and p.shape == (n,)
        assert np.array_equal(np.sort(p), np.arange(n)), (n, seed, epoch)


@pytest.mark.parametrize("n", SIZES)
def test_any_window_is_the_slice_of_the_whole(L, n):
    whole = L.host_indices(n, 5, 2)
    rng = np.random.Generator(np.random.PCG64(n))
    windows = [(0, 0), (0, n), (n, 0), (n - 1, 1), (0, 1)]                  # (first, count): empty, whole, empty at the end, last, first
    for _ in range(6):
        a, b = sorted(int(v) for v in rng.integers(0, n + 1, 2))
        windows.append((a, b - a))
    for first, count in windows:
        assert np.array_equal(L.host_indices(n, 5, 2, first, count), whole[first:first + count]), (n, first, count)


def test_epochs_and_seeds_give_unrelated_orders(big):
    assert int((big[0, 0] == big[0, 1]).sum()) <= 10          # epochs 0 and 1
    assert int((big[0, 0] == big[1, 0]).sum()) <= 10          # two seeds


def test_the_order_looks_shuffled(big):
    p, i = big[0, 0], np.arange(N_BIG)
    assert int((p == i).sum()) <= 10                          # fixed points
    assert int((np.abs(np.diff(p)) == 1).sum()) <= 12         # neighbours that stayed neighbours
    assert abs(float(np.corrcoef(i, p)[0, 1])) <= 0.02


def test_indices_host_argument_errors():
    import season_nerf_amd as sn
    lib = sn._lib.lib()
    out = np.zeros(8, dtype=np.int64)
    for n, epoch, first, count in ((0, 0, 0, 0), (10, -1, 0, 1), (10, 0, -1, 1), (10, 0, 8, 3), (10, 0, 0, -1)):
        assert lib.snerf_loader_indices_host(n, 0, epoch, first, count, out.ctypes.data) == -1, (n, epoch, first, count)
    assert lib.snerf_loader_indices_host(10, 0, 0, 0, 4, None) == -1
    assert b"snerf_loader_indices_host" in lib.snerf_last_error()


KAT = [([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ([0xffffffff] * 4, [0xffffffff] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(L, ctr, key, want):
    """Philox4x32-10's published vectors - through the generator itself, and through the sun-check rays, whose counter is (i, draws lo, draws hi, rank)
    and whose key is the seed: with bounds [0, 1] the ray coordinates ARE the uniforms (word >> 8) * 2^-24."""
    words = [int(w, 16) for w in want.split()]
    assert [int(x) for x in L.philox4x32_10(ctr, key)] == words
    seed = key[0] | (key[1] << 32)
    draws = ctr[1] | (ctr[2] << 32)
    draws = draws - (1 << 64) if draws >= 1 << 63 else draws          # the ABI takes int64: the same 64 bits
    rank = ctr[3] - (1 << 32) if ctr[3] >= 1 << 31 else ctr[3]
    top, bot = L.host_sc_rays(seed, draws, rank, ctr[0], 1, bounds=[[0, 1], [0, 1], [0, 1]])
    u = [np.float32(w >> 8) * np.float32(2.0 ** -24) for w in words]
    assert top[0].tolist() == [u[0], u[1], 1.0] and bot[0].tolist() == [u[2], u[3], 0.0]


def _sc_numpy(L, seed, draws, rank, first, count, bounds):
    """SC_loader.__getitem__ (NN_loaders/mg_SC_loader.py:17-21) restated in numpy float32: every product and every sum rounded on its own."""
    b = np.asarray(bounds, dtype=np.float32)
    dx, x0, dy, y0 = b[0, 1] - b[0, 0], b[0, 0], b[1, 1] - b[1, 0], b[1, 0]
    top, bot = np.empty((count, 3), np.float32), np.empty((count, 3), np.float32)
    for j in range(count):
        w = L.philox4x32_10([(first + j) & 0xffffffff, draws & 0xffffffff, (draws >> 32) & 0xffffffff, rank], [seed & 0xffffffff, seed >> 32])
        u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        top[j] = [np.float32(u[0] * dx) + x0, np.float32(u[1] * dy) + y0, b[2, 1]]
        bot[j] = [np.float32(u[2] * dx) + x0, np.float32(u[3] * dy) + y0, b[2, 0]]
    return top, bot


BOUNDS = [None, [[-0.75, 0.5], [-0.2, 0.9], [-0.6, 0.3]], [[0.1, 0.35], [-1.0, 1.0], [-1.0, 0.25]]]


@pytest.mark.parametrize("bounds", BOUNDS)
def test_sc_rays_match_the_numpy_restatement_bit_for_bit(L, bounds):
    b = [[-1, 1], [-1, 1], [-1, 1]] if bounds is None else bounds
    for seed, draws, rank, first, count in ((0, 0, 0, 0, 257), (12345678901234567, (1 << 32) + 5, 3, 1000, 64)):
        top, bot = L.host_sc_rays(seed, draws, rank, first, count, bounds)
        rt, rb = _sc_numpy(L, seed, draws, rank, first, count, b)
        assert top.tobytes() == rt.tobytes() and bot.tobytes() == rb.tobytes()
        assert np.all(top[:, 0] >= b[0][0]) and np.all(top[:, 0] <= b[0][1]) and np.all(top[:, 1] >= b[1][0]) and np.all(top[:, 1] <= b[1][1])
        assert np.all(bot[:, 0] >= b[0][0]) and np.all(bot[:, 0] <= b[0][1]) and np.all(bot[:, 1] >= b[1][0]) and np.all(bot[:, 1] <= b[1][1])
        assert np.all(top[:, 2] == np.float32(b[2][1])) and np.all(bot[:, 2] == np.float32(b[2][0]))
        assert len(np.unique(top[:, 0])) > count * 0.9        # (rays of one draw are not copies of each other)


def test_sc_rays_of_another_draw_or_rank_differ(L):
    base = L.host_sc_rays(3, 10, 0, 0, 128)
    for other in (L.host_sc_rays(3, 11, 0, 0, 128), L.host_sc_rays(3, 10, 1, 0, 128), L.host_sc_rays(4, 10, 0, 0, 128)):
        for a, b in zip(base, other):
            assert int((a[:, :2] == b[:, :2]).sum()) <= 2
    again = L.host_sc_rays(3, 10, 0, 0, 128)
    assert base[0].tobytes() == again[0].tobytes() and base[1].tobytes() == again[1].tobytes()
    win = L.host_sc_rays(3, 10, 0, 40, 8)                     # a window is the slice of the whole
    assert np.array_equal(win[0], base[0][40:48]) and np.array_equal(win[1], base[1][40:48])


def test_loader_create_argument_errors():
    """SNERF_E_INVALID before any launch or allocation: the table pointer is never dereferenced (no GPU here)."""
    import season_nerf_amd as sn
    lib = sn._lib.lib()
    table = C.c_void_p(0x1000)
    bad = {"n_rows < 1": (table, 0, 22, 4, 0, 0, 0, 1), "batch < 1": (table, 100, 22, 0, 0, 0, 0, 1),
           "batch * world > n_rows with drop_last": (table, 100, 22, 51, 0, 1, 0, 2), "batch > n_rows with drop_last": (table, 100, 22, 101, 0, 1, 0, 1),
           "world > 1 without drop_last": (table, 100, 22, 10, 0, 0, 0, 2), "rank < 0": (table, 100, 22, 10, 0, 1, -1, 2),
           "rank >= world": (table, 100, 22, 10, 0, 1, 2, 2), "world < 1": (table, 100, 22, 10, 0, 1, 0, 0),
           "row width 11": (table, 100, 11, 10, 0, 0, 0, 1), "row width 23": (table, 100, 23, 10, 0, 0, 0, 1), "NULL table": (None, 100, 22, 10, 0, 0, 0, 1)}
    for what, a in bad.items():
        h = C.c_void_p(0xdead)
        assert lib.snerf_loader_create(*a, None, C.byref(h)) == -1, what
        assert h.value is None, what                          # no handle comes back
        assert b"snerf_loader_create" in lib.snerf_last_error(), what
    assert lib.snerf_loader_create(table, 100, 22, 10, 0, 0, 0, 1, None, None) == -1
    lib.snerf_loader_destroy(None)                            # a no-op
    assert lib.snerf_loader_batches_per_epoch(None) == -1 and lib.snerf_loader_batch(None) == -1
    assert lib.snerf_loader_next(None, None, None) == -1
    s = (C.c_int64 * 4)()
    assert lib.snerf_loader_get_state(None, s, None) == -1 and lib.snerf_loader_set_state(None, s, None) == -1


def test_python_mirror_of_the_epoch_layout(L):
    assert L.epoch_batch_sizes(1000, 96) == [96] * 10 + [40] and L.batches_per_epoch(1000, 96) == 11
    assert L.epoch_batch_sizes(1000, 96, drop_last=True) == [96] * 10 and L.batches_per_epoch(1000, 96, True) == 10
    assert L.epoch_batch_sizes(1000, 96, drop_last=True, world=2) == [96] * 5 and L.batches_per_epoch(1000, 96, True, 2) == 5
    assert L.epoch_batch_sizes(1000, 1000) == [1000] and L.epoch_batch_sizes(1000, 1) == [1] * 1000
    assert L.epoch_batch_sizes(960, 96) == [96] * 10                       # no short batch: the same with and without drop_last
    assert L.epoch_batch_sizes(1, 4) == [1] and L.epoch_batch_sizes(5, 4) == [4, 1]
    for n, b in ((1000, 96), (4097, 64), (7, 7), (7, 3)):
        assert sum(L.epoch_batch_sizes(n, b)) == n and sum(L.epoch_batch_sizes(n, b, True)) == n // b * b


def test_loader_needs_a_device_table(L):
    import torch
    with pytest.raises(ValueError, match="GPU"):
        L.DeviceRayLoader(torch.zeros(10, 22), 4)
