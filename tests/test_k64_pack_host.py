"""CPU-only checks of the int8-digit stream laid out for v_mfma_i32_16x16x64_i8 (csrc/program.h "k64", csrc/pack.cpp pack_program_k64; program 5 of
snerf_model_pack_host): decoded with an independent Python statement of the layout rules and evaluated in exact integer arithmetic, it must reproduce the
network for the programs of all four variants (a variant runs a prefix of the layer list, so its program is a prefix of the stream); the k-slot order of
every k-step is a bijection; padded rows and slots carry zero digits; and the integers, scales and biases are those of the 32x32x32 stream (program 2)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import season_nerf_oracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, CN = 256, 4
CHUNK, PAIR, FRAG = 16384, 2048, 1024


@pytest.fixture(scope="module")
def lib():
    spec = importlib.util.spec_from_file_location("snerf_build", os.path.join(REPO, "season_nerf_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()
    b.build_ops()
    import season_nerf_amd as sn
    return sn._lib.lib()


# ---- the layout rules, restated
def slot_H(s, g, j):
    """hidden k-step s, lane group g, byte j: four consecutive 16-row output blocks b = j // 4 of the producer, rows 4 g + j % 4"""
    return 64 * s + 16 * (j // 4) + 4 * g + j % 4


def slot_pepos(s, g, j):
    """PE(pos), one k-step: the 30 (coordinate, frequency) pairs in order, eight per lane group; cos in the even byte, sin in the odd one.
    Reference feature order: [x0 x1 x2 | per d: cos(k_0..k_9 x_d), sin(k_0..k_9 x_d)]; the raw coordinates have no slot."""
    p = 8 * g + j // 2
    return 3 + 20 * (p // 10) + 10 * (j & 1) + p % 10 if s == 0 and p < 30 else -1


def slot_pesun(s, g, j):
    """PE(sun), one k-step: the 12 pairs p = 4 d + f, three per lane group in bytes 0..5"""
    p = 3 * g + j // 2
    return 3 + 8 * (p // 4) + 4 * (j & 1) + p % 4 if s == 0 and j < 6 else -1


# (name, real rows, padded rows, hidden k-steps, encoding) in stream order; variant v runs the first N_LAYERS[v] of them
W2 = W // 2
LAYERS = ([("fc1", W, W, 0, "pos")] + [(f"fc{i}", W, W, W // 64, None) for i in (2, 3, 4)] + [("fc5", W, W, W // 64, "pos")]
          + [(f"fc{i}", W, W, W // 64, None) for i in (6, 7, 8)] + [("fc9", W2, W2, W // 64, None), ("head", 4, 16, W2 // 64, None),
             ("s1", W2, W2, W2 // 64, "sun"), ("s2", W2, W2, W2 // 64, None), ("s3", W2, W2, W2 // 64, None), ("s4", 1, 16, W2 // 64, None),
             ("a1", W, W, W2 // 64, None), ("a2", W, W, W // 64, None), ("a3", W, W, W // 64, None), ("ac", 3 * CN, 16, W // 64, None)])
N_LAYERS = {0: 18, 1: 14, 2: 10, 3: 10}


class Model:
    def __init__(self, lib):
        self.lib = lib
        self.sd = orc.init_weights(W, CN, seed=7)
        self.m = lib.snerf_model_create(W, CN)
        assert lib.snerf_model_set_precision(self.m, 2) == 0
        for k, v in self.sd.items():
            if v.is_floating_point():
                arr = np.ascontiguousarray(v.numpy())
                assert lib.snerf_model_set_tensor(self.m, k.encode(), arr.ctypes.data, arr.size) == 0

    def packed(self, program):
        ns, nb = C.c_size_t(), C.c_size_t()
        assert self.lib.snerf_model_pack_host(self.m, program, None, C.byref(ns), None, C.byref(nb)) == 0
        stream, tab = np.zeros(ns.value, dtype=np.int8), np.zeros(nb.value, dtype=np.float32)
        assert self.lib.snerf_model_pack_host(self.m, program, stream.ctypes.data, C.byref(ns), tab.ctypes.data, C.byref(nb)) == 0
        return stream, tab


@pytest.fixture(scope="module")
def model(lib):
    m = Model(lib)
    yield m
    lib.snerf_model_destroy(m.m)


def decode(stream, tab):
    """per layer: digit matrices T, L [padded rows, 64 * k-steps] in slot order (slot = 64 s + 16 g + j), scale, bias, raw weights [rows, 3] or None"""
    out, chunk, toff = {}, 0, 0
    for name, n_ref, n_pad, kh, enc in LAYERS:
        ks, nb = kh + (1 if enc else 0), n_pad // 16
        T = np.zeros((n_pad, 64 * ks), dtype=np.int64)
        L = np.zeros((n_pad, 64 * ks), dtype=np.int64)
        for b in range(nb):
            for s in range(ks):
                o = chunk * CHUNK + (b * ks + s) * PAIR
                t = stream[o:o + FRAG].reshape(64, 16)
                l = stream[o + FRAG:o + PAIR].reshape(64, 16)
                for lane in range(64):
                    r, g = lane % 16, lane // 16
                    T[16 * b + r, 64 * s + 16 * g:64 * s + 16 * g + 16] = t[lane]
                    L[16 * b + r, 64 * s + 16 * g:64 * s + 16 * g + 16] = l[lane]
        sc, bi = np.zeros(n_pad), np.zeros(n_pad)
        for b in range(nb):
            for g in range(4):
                for i in range(4):
                    sc[16 * b + 4 * g + i] = tab[toff + (b * 4 + g) * 8 + i]
                    bi[16 * b + 4 * g + i] = tab[toff + (b * 4 + g) * 8 + 4 + i]
        toff += 2 * n_pad
        Wraw = None
        if enc:
            Wraw = np.zeros((n_pad, 3))
            for b in range(nb):
                for g in range(4):
                    for i in range(4):
                        for dd in range(3):
                            Wraw[16 * b + 4 * g + i, dd] = tab[toff + ((b * 4 + g) * 3 + dd) * 4 + i]
            toff += 3 * n_pad
        out[name] = (T, L, sc, bi, Wraw)
        chunk += -(-(nb * ks) // 8)              # every layer starts on a chunk
    assert chunk * CHUNK == len(stream) and toff == len(tab)
    return out


def variant_prefix(variant):
    """bytes of the stream a variant's program consumes per tile"""
    return sum(-(-((n_pad // 16) * (kh + (1 if enc else 0))) // 8) for _, _, n_pad, kh, enc in LAYERS[:N_LAYERS[variant]]) * CHUNK


def gather(feat, slot_fn, ks):
    out = np.zeros((feat.shape[0], 64 * ks))
    for s in range(ks):
        for g in range(4):
            for j in range(16):
                f = slot_fn(s, g, j)
                if 0 <= f < feat.shape[1]:
                    out[:, 64 * s + 16 * g + j] = feat[:, f]
    return out


def layer(x_slots, T, L, sc, bi, Wraw=None, raw=None):
    q = np.rint(np.clip(x_slots, -1, 1) * 32767).astype(np.int64)
    a = q >> 8
    b = (q & 255) - 128
    acc = 256 * (a @ T.T) + b @ T.T + a @ L.T
    assert np.abs(acc).max() < 2 ** 31
    z = acc.astype(np.float64) * sc + bi
    return z if Wraw is None else z + raw @ Wraw.T


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_k64_stream_reproduces_the_network(model, variant):
    """exact integer arithmetic on the decoded digits against the oracle in float64, over the layers the variant runs"""
    stream, tab = model.packed(5)
    D = decode(stream, tab)
    assert variant_prefix(0) == len(stream) and 0 < variant_prefix(variant) <= len(stream)
    rng = np.random.Generator(np.random.PCG64(3))
    N = 48
    X = torch.tensor(rng.uniform(-1.7, 1.7, (N, 3)))        # beyond the cube: the raw coordinates must not saturate
    sun = rng.uniform(0, 1, (N, 3)); sun /= np.linalg.norm(sun, axis=1, keepdims=True)
    sun = torch.tensor(sun)
    tim = torch.tensor(rng.uniform(-1, 1, (N, 4)))
    with torch.no_grad():
        ref = orc.forward_separate(orc.cast_weights(model.sd, torch.float64), X, sun, tim)
        pe_pos = orc.pe_encode(X, 10).numpy()
        pe_sun = orc.pe_encode(sun, 4).numpy()
    act = lambda z: np.sin(2 * np.pi * z)
    Xn, Sn = X.numpy(), sun.numpy()
    KW, KW2 = W // 64, W2 // 64
    run = set(n for n, *_ in LAYERS[:N_LAYERS[variant]])
    P = gather(pe_pos, slot_pepos, 1)
    h = act(layer(P, *D["fc1"], raw=Xn))
    for n in ("fc2", "fc3", "fc4"):
        h = act(layer(gather(h, slot_H, KW), *D[n]))
    h = act(layer(np.concatenate([gather(h, slot_H, KW), P], 1), *D["fc5"], raw=Xn))
    for n in ("fc6", "fc7", "fc8"):
        h = act(layer(gather(h, slot_H, KW), *D[n]))
    x1 = act(layer(gather(h, slot_H, KW), *D["fc9"]))
    head = layer(gather(x1, slot_H, KW2), *D["head"])
    tol = dict(rtol=5e-4, atol=2e-4)      # 16-bit fixed point on both operands, fourteen layers deep (the tolerance of the 32x32x32 stream's test)
    np.testing.assert_allclose(head[:, 0:3], ref[1].numpy(), **tol)                                   # Col_raw
    np.testing.assert_allclose(np.log1p(np.exp(head[:, 3:4])), ref[0].numpy(), **tol)                 # Rho
    if "s4" in run:
        a = act(layer(np.concatenate([gather(x1, slot_H, KW2), gather(pe_sun, slot_pesun, 1)], 1), *D["s1"], raw=Sn))
        for n in ("s2", "s3"):
            a = act(layer(gather(a, slot_H, KW2), *D[n]))
        sv = layer(gather(a, slot_H, KW2), *D["s4"])
        np.testing.assert_allclose(1 / (1 + np.exp(-sv[:, 0:1])), ref[2].numpy(), **tol)              # Solar_Vis
    if "ac" in run:
        y = act(layer(gather(x1, slot_H, KW2), *D["a1"]))
        for n in ("a2", "a3"):
            y = act(layer(gather(y, slot_H, KW), *D[n]))
        adj = layer(gather(y, slot_H, KW), *D["ac"])
        np.testing.assert_allclose(adj[:, :3 * CN].reshape(N, CN, 3), ref[5].numpy(), **tol)          # output i is row i


def test_k_slot_order_is_a_bijection_per_k_step():
    """hidden k-step s: the 64 slots are exactly features 64 s .. 64 s + 63; the encodings' k-steps hit every digit feature once and no raw coordinate"""
    for s in range(W // 64):
        feats = sorted(slot_H(s, g, j) for g in range(4) for j in range(16))
        assert feats == list(range(64 * s, 64 * s + 64))
    pos = [slot_pepos(0, g, j) for g in range(4) for j in range(16)]
    assert sorted(f for f in pos if f >= 0) == list(range(3, 63)) and pos.count(-1) == 4
    sun = [slot_pesun(0, g, j) for g in range(4) for j in range(16)]
    assert sorted(f for f in sun if f >= 0) == list(range(3, 27)) and sun.count(-1) == 40
    assert all(slot_pepos(1, g, j) == -1 and slot_pesun(1, g, j) == -1 for g in range(4) for j in range(16))


def test_padded_rows_and_slots_carry_zero_digits(model):
    D = decode(*model.packed(5))
    for name, real in (("head", 4), ("s4", 1), ("ac", 3 * CN)):          # rows 4..15, 1..15, 12..15
        T, L, sc, bi, _ = D[name]
        assert T.shape[0] == 16
        assert not T[real:].any() and not L[real:].any() and not sc[real:].any() and not bi[real:].any(), name
        assert T[:real].any()
    # fc_solar_1: K = 128 + 27 = 155 real inputs in 3 x 64 slots: the encoding's k-step holds 24 digit features, so slots 155..191 of the padded K - and, in
    # slot order, every slot of k-step 2 that maps to no feature - are zero
    T, L, _, _, Wraw = D["s1"]
    pads = [128 + 16 * g + j for g in range(4) for j in range(16) if slot_pesun(0, g, j) < 0]
    assert len(pads) == 40 and not T[:, pads].any() and not L[:, pads].any()
    assert T.shape[1] == 192 and Wraw[:, :3].any()
    # fc1: K = 63 real inputs, 60 of them digits: four pad slots of the one k-step (63 of a 64-slot k-step and the raw coordinates' three)
    T, L, _, _, Wraw = D["fc1"]
    pads = [16 * g + j for g in range(4) for j in range(16) if slot_pepos(0, g, j) < 0]
    assert pads == [60, 61, 62, 63] and not T[:, pads].any() and not L[:, pads].any() and Wraw.any()
    # fc5's encoding k-step likewise
    T, L, _, _, _ = D["fc5"]
    assert T.shape[1] == 320 and not T[:, 316:].any() and not L[:, 316:].any()


def test_same_integers_scales_and_biases_as_the_32x32x32_stream(model):
    """every real row's multiset of (T, L) digit pairs, its scale and its bias are those of program 2 (the old stream): estimate_i8 and its bound hold unchanged"""
    D = decode(*model.packed(5))
    s2, t2 = model.packed(2)
    acc_row = lambda i, h: (i & 3) + 8 * (i >> 2) + 4 * h
    chunk, toff = 0, 0
    for name, n_ref, n_pad, kh, enc in LAYERS:
        n32 = max(n_pad, 32)
        ks = 2 * kh + ({"pos": 2, "sun": 1}.get(enc, 0))
        nb = n32 // 32
        T = np.zeros((n32, 32 * ks), dtype=np.int64)
        L = np.zeros((n32, 32 * ks), dtype=np.int64)
        for b in range(nb):
            for s in range(ks):
                o = chunk * CHUNK + (b * ks + s) * PAIR
                t = s2[o:o + FRAG].reshape(64, 16)
                l = s2[o + FRAG:o + PAIR].reshape(64, 16)
                for lane in range(64):
                    T[32 * b + lane % 32, 32 * s + 16 * (lane // 32):32 * s + 16 * (lane // 32) + 16] = t[lane]
                    L[32 * b + lane % 32, 32 * s + 16 * (lane // 32):32 * s + 16 * (lane // 32) + 16] = l[lane]
        sc, bi = np.zeros(n32), np.zeros(n32)
        for b in range(nb):
            for h in range(2):
                for i in range(16):
                    sc[32 * b + acc_row(i, h)] = t2[toff + (b * 2 + h) * 32 + i]
                    bi[32 * b + acc_row(i, h)] = t2[toff + (b * 2 + h) * 32 + 16 + i]
        toff += (5 if enc else 2) * n32
        chunk += -(-(nb * ks) // 8)
        # the old stream maps the adjust head's output i to accumulator register i of lane-half 0; every other layer is the identity
        old_row = (lambda i: acc_row(i, 0)) if name == "ac" else (lambda i: i)
        Tn, Ln, scn, bin_, _ = D[name]
        for i in range(n_ref):
            o = old_row(i)
            assert scn[i] == np.float32(sc[o]) and bin_[i] == np.float32(bi[o]), (name, i)
            new = sorted(zip(Tn[i][(Tn[i] != 0) | (Ln[i] != 0)], Ln[i][(Tn[i] != 0) | (Ln[i] != 0)]))
            old = sorted(zip(T[o][(T[o] != 0) | (L[o] != 0)], L[o][(T[o] != 0) | (L[o] != 0)]))
            assert new == old, (name, i)


def test_program_5_exists_only_for_the_int8_mode_at_width_256(lib):
    n = C.c_size_t()
    m = lib.snerf_model_create(W, CN)
    assert lib.snerf_model_pack_host(m, 5, None, C.byref(n), None, None) == -4       # SNERF_E_STATE without the precision mode
    lib.snerf_model_destroy(m)
    m = lib.snerf_model_create(64, CN)
    assert lib.snerf_model_set_precision(m, 2) == 0
    assert lib.snerf_model_pack_host(m, 5, None, C.byref(n), None, None) == -4       # W = 64 stays on the 32x32x32 stream
    lib.snerf_model_destroy(m)
