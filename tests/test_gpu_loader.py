"""loader.DeviceRayLoader on the GPU: the gather against the host mirror of the permutation (exact: the table's entries encode (row, column)), epoch ends,
ranks, the sun-check rays bit for bit, the position in device memory (state, resume, a draw captured in a graph), the custom op, and training through
GraphedTrainStep(tool, loader=...) / T_NeRF_Net_Tool(train_loader=...).

Every draw of the gather tests lands in ONE flat arena whose outputs are separated by sentinel gaps; the whole arena is compared with an expected image built
on the host, so a write outside an output, into an output that was not asked for, or past the rows of a short batch fails the same comparison."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_net_tool import _args

pytestmark = pytest.mark.gpu

N = 1000
COLS = {"Img_Pt": (0, 2), "Top": (2, 5), "Bot": (5, 8), "View_Angle": (8, 11), "Sun_Angle": (11, 14), "Time_Encoded": (14, 18), "Sample_Weight": (18, 19),
        "GT_Color": (19, 22)}
FLOAT_OUTS = list(COLS) + ["SC_Top", "SC_Bot"]
SENT, GAP = -7777.0, 64
WC, H4 = np.array([41.29, -95.9, 300.0]), np.array([[310.0, 12.0, 0.0, -11650.0], [-9.0, 240.0, 0.0, 23390.0], [0.0, 0.0, 0.01, -3.0], [0, 0, 0, 1.0]])


def _table_np(n=N):
    return (np.arange(n, dtype=np.float32)[:, None] * 32 + np.arange(22, dtype=np.float32)[None, :])       # exact in fp32: < 2^24


@pytest.fixture(scope="module")
def table():
    t = torch.from_numpy(_table_np()).cuda()
    yield t
    assert np.array_equal(t.cpu().numpy(), _table_np())          # nobody wrote into the table


class Arena:
    """Fixed output buffers with sentinels on both sides of each: one flat float tensor (gap | out | gap | out | ... | gap) + the int64 index buffer."""

    def __init__(self, B, names=FLOAT_OUTS, index=True):
        self.B, self.names, self.off = B, list(names), {}
        o = GAP
        for k in self.names:
            w = 3 if k.startswith("SC_") else COLS[k][1] - COLS[k][0]
            self.off[k] = (o, w)
            o += B * w + GAP
        self.flat = torch.full((o,), SENT, device="cuda")
        self.bufs = {k: self.flat[a:a + B * w].view(B, w) for k, (a, w) in self.off.items()}
        self.idx = torch.full((B + 2 * GAP,), -5, dtype=torch.int64, device="cuda") if index else None
        if index:
            self.bufs["Row_Index"] = self.idx[GAP:GAP + B]

    def reset(self):
        self.flat.fill_(SENT)
        if self.idx is not None:
            self.idx.fill_(-5)

    def snapshot(self):
        return self.flat.clone(), (self.idx.clone() if self.idx is not None else None)

    def expected(self, tab, idx, sc=None):
        """The arena after a draw of rows `idx` (and sun-check rays `sc` = (top, bot)): everything else is sentinel."""
        flat = np.full(self.flat.numel(), SENT, dtype=np.float32)
        rows = len(idx)
        for k, (a, w) in self.off.items():
            if k.startswith("SC_"):
                if sc is None:
                    raise AssertionError("sun-check rays expected")
                v = sc[0] if k == "SC_Top" else sc[1]
            else:
                v = tab[idx][:, COLS[k][0]:COLS[k][1]]
            flat[a:a + rows * w] = np.ascontiguousarray(v, dtype=np.float32).reshape(-1)
        ix = np.full(self.B + 2 * GAP, -5, dtype=np.int64)
        ix[GAP:GAP + rows] = idx
        return flat, ix


def _loader(table, B, **kw):
    import season_nerf_amd as sn
    return sn.DeviceRayLoader(table, B, **kw)


def _run_epochs(ld, arena, n_draws):
    """n_draws draws into the arena -> [(rows, flat, idx)] as numpy (one device -> host copy per draw, after all draws were queued)."""
    snaps = []
    for _ in range(n_draws):
        arena.reset()
        rows = ld.next_into(arena.bufs)
        snaps.append((rows,) + arena.snapshot())
    return [(r, f.cpu().numpy(), None if i is None else i.cpu().numpy()) for r, f, i in snaps]


@pytest.mark.parametrize("B", [1, 96, 1000])
def test_a_whole_epoch_is_every_row_once_in_the_host_order(table, B):
    from season_nerf_amd import loader as L
    seed = 3
    ld, arena, tab = _loader(table, B, seed=seed), Arena(B), _table_np()
    sizes = L.epoch_batch_sizes(N, B)
    assert len(ld) == len(sizes) and ld.graph_safe == (N % B == 0)
    perm = L.host_indices(N, seed, 0)
    got, pos = [], 0
    for d, (rows, flat, idx) in enumerate(_run_epochs(ld, arena, len(sizes))):
        assert rows == sizes[d]
        want = perm[pos:pos + rows]
        ef, ei = arena.expected(tab, want, L.host_sc_rays(seed, d, 0, 0, rows))
        assert np.array_equal(idx, ei), (B, d)
        assert flat.tobytes() == ef.tobytes(), (B, d, np.flatnonzero(flat != ef)[:8])
        got.append(idx[GAP:GAP + rows])
        pos += rows
    assert np.array_equal(np.sort(np.concatenate(got)), np.arange(N))
    assert ld.get_state() == (1, 0, len(sizes))


def test_short_last_batch_then_a_new_order(table):
    """1000 = 10 x 96 + 40: the eleventh batch has 40 rows (the other 56 rows of every buffer untouched), the twelfth opens epoch 1 with another order."""
    from season_nerf_amd import loader as L
    ld, arena, tab = _loader(table, 96, seed=9), Arena(96), _table_np()
    out = _run_epochs(ld, arena, 12)
    assert [r for r, _, _ in out] == [96] * 10 + [40, 96]
    p0, p1 = L.host_indices(N, 9, 0), L.host_indices(N, 9, 1)
    for d, want in ((10, p0[960:]), (11, p1[:96])):
        ef, ei = arena.expected(tab, want, L.host_sc_rays(9, d, 0, 0, len(want)))
        assert np.array_equal(out[d][2], ei) and out[d][1].tobytes() == ef.tobytes(), d
    assert not np.array_equal(p1[:96], p0[:96])
    assert ld.get_state() == (1, 1, 12)
    d = ld.next()                                              # next(): fresh tensors, the reference's keys
    assert sorted(d) == sorted(FLOAT_OUTS) and all(v.shape[0] == 96 and v.is_contiguous() for v in d.values())
    assert np.array_equal(d["GT_Color"].cpu().numpy(), tab[p1[96:192]][:, 19:22])


def test_drop_last_gives_ten_full_batches(table):
    from season_nerf_amd import loader as L
    ld, arena, tab = _loader(table, 96, seed=9, drop_last=True), Arena(96), _table_np()
    assert len(ld) == 10 and ld.graph_safe
    out = _run_epochs(ld, arena, 11)
    assert [r for r, _, _ in out] == [96] * 11
    p0, p1 = L.host_indices(N, 9, 0), L.host_indices(N, 9, 1)
    for d, want in ((9, p0[864:960]), (10, p1[:96])):
        ef, ei = arena.expected(tab, want, L.host_sc_rays(9, d, 0, 0, 96))
        assert np.array_equal(out[d][2], ei) and out[d][1].tobytes() == ef.tobytes(), d
    assert ld.get_state() == (1, 1, 11)


def test_null_outputs_are_skipped(table):
    """Only Top, GT_Color and SC_Bot are asked for, without the index: the other outputs' memory (here: the gaps of a smaller arena) stays untouched."""
    from season_nerf_amd import loader as L
    names = ["Top", "GT_Color", "SC_Bot"]
    ld, arena, tab = _loader(table, 96, seed=2), Arena(96, names, index=False), _table_np()
    (rows, flat, _), = _run_epochs(ld, arena, 1)
    ef, _ = arena.expected(tab, L.host_indices(N, 2, 0, 0, 96), L.host_sc_rays(2, 0, 0, 0, 96))
    assert rows == 96 and flat.tobytes() == ef.tobytes()
    assert ld.next_into({}) == 96 and ld.get_state() == (0, 2, 2)           # nothing asked for: the position still advances
    with pytest.raises(ValueError, match="unknown"):
        ld.next_into({"Colour": arena.bufs["Top"]})


@pytest.mark.parametrize("B,drop_last", [(1, False), (4, False), (1, True)])
def test_a_table_of_one_row(B, drop_last):
    tab = _table_np(1)
    t = torch.from_numpy(tab).cuda()
    ld, arena = _loader(t, B, seed=1, drop_last=drop_last), Arena(B)
    from season_nerf_amd import loader as L
    for d, (rows, flat, idx) in enumerate(_run_epochs(ld, arena, 3)):
        ef, ei = arena.expected(tab, np.zeros(1, dtype=np.int64), L.host_sc_rays(1, d, 0, 0, 1))
        assert rows == 1 and np.array_equal(idx, ei) and flat.tobytes() == ef.tobytes()
    assert ld.get_state() == (3, 0, 3)


def test_two_ranks_take_disjoint_blocks_of_one_permutation(table):
    from season_nerf_amd import loader as L
    perm, tab = L.host_indices(N, 4, 0), _table_np()
    seen = []
    for rank in (0, 1):
        ld, arena = _loader(table, 96, seed=4, drop_last=True, rank=rank, world=2), Arena(96)
        assert len(ld) == 5
        for k, (rows, flat, idx) in enumerate(_run_epochs(ld, arena, 5)):
            want = perm[(k * 2 + rank) * 96:(k * 2 + rank + 1) * 96]
            ef, ei = arena.expected(tab, want, L.host_sc_rays(4, k, rank, 0, 96))
            assert rows == 96 and np.array_equal(idx, ei) and flat.tobytes() == ef.tobytes(), (rank, k)
            seen.append(idx[GAP:GAP + 96])
        assert ld.get_state() == (1, 0, 5)
    seen = np.concatenate(seen)
    assert len(np.unique(seen)) == 960 and np.array_equal(np.sort(seen), np.sort(perm[:960]))
    import season_nerf_amd as sn
    with pytest.raises(RuntimeError, match="drop_last"):
        sn.DeviceRayLoader(table, 96, rank=0, world=2)


@pytest.mark.parametrize("bounds", [[[-0.75, 0.5], [-0.2, 0.9], [-0.6, 0.3]], [[0.1, 0.35], [-1.0, 1.0], [-1.0, 0.25]]])
def test_sun_check_rays_equal_the_host_mirror_bit_for_bit(table, bounds):
    from season_nerf_amd import loader as L
    seed = 12345678901234567
    ld, arena = _loader(table, 96, seed=seed, drop_last=True, rank=1, world=2, bounds=torch.tensor(bounds)), Arena(96, ["SC_Top", "SC_Bot"], index=False)
    for d, (rows, flat, _) in enumerate(_run_epochs(ld, arena, 3)):
        top, bot = L.host_sc_rays(seed, d, 1, 0, 96, bounds)
        ef, _ = arena.expected(None, np.zeros(96, dtype=np.int64), (top, bot))
        assert flat.tobytes() == ef.tobytes(), d
        assert top[:, 0].min() >= bounds[0][0] and top[:, 0].max() <= bounds[0][1] and np.all(top[:, 2] == np.float32(bounds[2][1]))


def test_resume_mid_epoch_continues_with_the_same_batches(table):
    a = _loader(table, 96, seed=6)
    for _ in range(7):
        a.next()
    st = a.state_dict()
    assert st == {"seed": 6, "epoch": 0, "batch": 7, "draws": 7}
    b = _loader(table, 96, seed=6)
    b.load_state_dict(st)
    for d in range(6):                                         # through the short batch and the epoch's end
        x, y = a.next(), b.next()
        assert x["Top"].shape[0] == y["Top"].shape[0] == (40 if d == 3 else 96)
        for k in x:
            assert torch.equal(x[k], y[k]), (d, k)
    assert a.get_state() == b.get_state() == (1, 2, 13)
    with pytest.raises(ValueError, match="seed"):
        _loader(table, 96, seed=7).load_state_dict(st)
    with pytest.raises(RuntimeError, match="set_state"):
        b.set_state(0, 11, 0)                                  # batch_in_epoch outside [0, 11)


def test_state_after_k_draws_equals_the_shadow(table):
    """The device copy of the position follows the rule of the host shadow: k draws -> (k // batches, k % batches, k)."""
    ld = _loader(table, 96, seed=0)
    for k in range(1, 25):
        ld.next_into({})
        if k in (1, 10, 11, 12, 22, 24):
            assert ld.get_state() == (k // 11, k % 11, k)


def test_custom_op_under_opcheck(table):
    import season_nerf_amd as sn
    ld, arena = _loader(table, 96, seed=1, drop_last=True), Arena(96)
    order = sorted(sn.loader.FIELDS, key=lambda k: sn.loader.FIELDS[k][0])
    args = (ld._handle, table) + tuple(arena.bufs[k] for k in order)
    torch.library.opcheck(torch.ops.season_nerf.loader_next.default, args, test_utils=("test_schema", "test_faketensor"))
    some = (ld._handle, table) + tuple(arena.bufs[k] if k in ("Top", "Row_Index") else None for k in order)
    torch.library.opcheck(torch.ops.season_nerf.loader_next.default, some, test_utils=("test_schema", "test_faketensor"))
    ops = sn.ops.load()
    with pytest.raises(RuntimeError, match="top"):
        ops.loader_next(ld._handle, table, None, arena.bufs["Top"][:50], *([None] * 9))           # fewer rows than a batch
    with pytest.raises(RuntimeError, match="gt_color"):
        ops.loader_next(ld._handle, table, *([None] * 7), arena.bufs["Top"][:, :2].contiguous(), None, None, None)
    with pytest.raises(RuntimeError, match="row_index"):
        ops.loader_next(ld._handle, table, *([None] * 8), arena.bufs["Row_Index"].int(), None, None)
    with pytest.raises(RuntimeError, match="table"):
        ops.loader_next(ld._handle, table[:, :21].contiguous(), *([None] * 11))


def test_solar_vecs_and_distances(table):
    """solar_vecs = the distinct Sun_Angle rows; with a DSM_Distance the dict carries get_Dist's two distances of the batch's own rays."""
    import season_nerf_amd as sn
    rng = np.random.Generator(np.random.PCG64(8))
    tab = _ray_table(rng, 300)
    suns = tab[:3, 11:14].copy()
    tab[:, 11:14] = suns[rng.integers(0, 3, 300)]
    hm = rng.uniform(-0.8, 0.6, (24, 24))
    dist = sn.DSM_Distance(hm, hm * 0.9, 32, "cuda")
    ld = sn.DeviceRayLoader(torch.from_numpy(tab).cuda(), 64, seed=2, dsm_distance=dist)
    assert np.array_equal(ld.solar_vecs, np.unique(suns, axis=0))
    d = ld.next()
    assert sorted(d) == sorted(FLOAT_OUTS + ["Dist_to_Surf_GT", "Dist_to_Surf_Prior"])
    gt, prior = dist.get_Dist(d["Top"], d["Bot"])
    assert torch.equal(torch.nan_to_num(d["Dist_to_Surf_GT"], nan=-1.0), torch.nan_to_num(gt, nan=-1.0)) and d["Dist_to_Surf_GT"].shape == (64, 1)
    assert torch.equal(torch.nan_to_num(d["Dist_to_Surf_Prior"], nan=-1.0), torch.nan_to_num(prior, nan=-1.0))


def test_a_captured_draw_advances_at_every_replay(table):
    """next_into captured ALONE in a graph and replayed 25 times (two epoch ends at 10 batches per epoch): replay j leaves what draw j of an eager loader with
    the same seed leaves - the position is read from, and advanced in, device memory; nothing about it is frozen into the graph."""
    g_ld, e_ld = _loader(table, 96, seed=11, drop_last=True), _loader(table, 96, seed=11, drop_last=True)
    ga, ea = Arena(96), Arena(96)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_ld.next_into(ga.bufs)
    assert g_ld.get_state() == (0, 0, 0)                       # a capture executes nothing
    snaps = []
    for _ in range(25):
        ga.reset()
        graph.replay()
        snaps.append(ga.snapshot())
    want = _run_epochs(e_ld, ea, 25)
    firsts = set()
    for j, ((flat, idx), (_, ef, ei)) in enumerate(zip(snaps, want)):
        assert flat.cpu().numpy().tobytes() == ef.tobytes() and np.array_equal(idx.cpu().numpy(), ei), j
        firsts.add(int(ei[GAP]))
    assert len(firsts) > 20                                    # (the eager draws themselves moved on)
    assert g_ld.get_state() == e_ld.get_state() == (2, 5, 25)
    x, y = g_ld.next(), e_ld.next()                            # an eager draw after the replays continues from the device's position
    assert all(torch.equal(x[k], y[k]) for k in x)
    bad = _loader(table, 96, seed=11)                          # a short last batch: not for a graph
    assert not bad.graph_safe


def _ray_table(rng, n):
    sun = rng.uniform(0.1, 1, (n, 3)); sun /= np.linalg.norm(sun, axis=1, keepdims=True)
    view = rng.uniform(-1, 1, (n, 3)); view /= np.linalg.norm(view, axis=1, keepdims=True)
    tau = rng.uniform(0, 1, (n, 2))
    time = np.stack([np.cos(6.28 * tau[:, 0]), np.sin(6.28 * tau[:, 0]), np.cos(6.28 * tau[:, 1]), np.sin(6.28 * tau[:, 1])], 1)
    return np.concatenate([rng.integers(0, 64, (n, 2)), rng.uniform(-1, 1, (n, 2)), np.ones((n, 1)), rng.uniform(-1, 1, (n, 2)), -np.ones((n, 1)), view, sun, time,
                           np.ones((n, 1)), rng.uniform(0, 1, (n, 3))], 1).astype(np.float32)


def test_captured_steps_that_draw_inside_the_graph_follow_eager_steps_fed_by_a_loader():
    """The set-up of test_graphed_train_step_follows_the_eager_step (W = 64, R = 96, S = 32, eight steps, MSE loss, free phase) with the batches drawn from a
    1000-row table: GraphedTrainStep(tool, loader=...) - two eager warm-up steps, then six replays whose first two kernels draw the batch - against eager steps
    fed by a second loader with the same seed.  That test's tolerances: losses within 2e-4 * max(|v|, 1e-3), parameters within 0.02 of the distance moved."""
    import season_nerf_amd as sn
    from oracle import season_nerf_oracle as orc
    W, R, S, n_steps = 64, 96, 32, 8
    tab = torch.from_numpy(_ray_table(np.random.Generator(np.random.PCG64(5)), N)).cuda()

    def run(graphed):
        net = sn.T_NeRF(W, 4)
        net.load_state_dict(orc.init_weights(W, 4, 7, bn_stats="identity"))
        net = net.cuda().train()
        args = SimpleNamespace(n_samples=S, Use_Reg=True, Solar_Type_2=False, Use_MSE_loss=True, Use_Solar=True, sc_lambda=0.03, number_low_frequency_cases=4)
        ev = sn.All_in_One_Eval(args, torch.device("cuda"), 10, False, None, H4, WC)
        tool = sn.Net_tool(net, ev, 3e-4, total_steps=n_steps + 1, lr_alpha_scale=30.0, writer=None)
        ld = sn.DeviceRayLoader(tab, R, seed=21, drop_last=True)
        assert sn.GraphedTrainStep.eligible(tool, ld) is None
        step = sn.GraphedTrainStep(tool, loader=ld, warmup=2) if graphed else None
        np.random.seed(11); torch.manual_seed(11)
        losses = []
        for k in range(n_steps):
            loss = step(None, k) if graphed else tool.train_step(ld.next(), k)
            losses.append({n: float(v[0]) for n, v in loss.items()})
        if graphed:
            assert step.graph is not None and step.calls == n_steps
        assert ld.get_state() == (0, n_steps, n_steps)
        return losses, {k: v.detach().clone() for k, v in net.state_dict().items()}, tool.sched.get_last_lr()[0]

    le, pe, lre = run(False)
    lg, pg, lrg = run(True)
    assert lre == lrg
    assert len({round(l["Color"], 9) for l in le}) == n_steps                          # (eight different batches)
    for k in range(n_steps):
        for n, v in le[k].items():
            print(f"  step {k} {n}: eager {v:.8e} captured {lg[k][n]:.8e}")
            assert abs(lg[k][n] - v) <= 2e-4 * max(abs(v), 1e-3), (k, n, lg[k][n], v)
    p0 = orc.init_weights(W, 4, 7, bn_stats="identity")
    moved = diff = 0.0
    for k, v in pe.items():
        if v.is_floating_point() and "running" not in k:
            moved += float((v.cpu() - p0[k]).abs().sum())
            diff += float((pg[k] - v).abs().sum())
        elif not v.is_floating_point():
            assert torch.equal(pg[k], v), k
    print(f"  drawn inside the graph vs eager after {n_steps} steps: sum |difference| / sum |update| = {diff / moved:.2e}")
    assert moved > 0 and diff < 0.02 * moved, (diff, moved)


def test_net_tool_trains_from_loaders_without_a_get_data_callable():
    """T_NeRF_Net_Tool(train_loader=, val_loader=, use_graph=True): 12 steps - the DSM-prior phase (2 steps, both eager warm-up), then the free phase (2 eager, 8
    replays that draw inside the graph); the validation batches of the two save points come from val_loader.  Without loaders and callable: as before."""
    import season_nerf_amd as sn
    from oracle import season_nerf_oracle as orc
    rng = np.random.Generator(np.random.PCG64(3))
    hm = rng.uniform(-0.8, 0.6, (24, 24))
    tab, vtab = torch.from_numpy(_ray_table(rng, 500)).cuda(), torch.from_numpy(_ray_table(rng, 200)).cuda()
    train, val = sn.DeviceRayLoader(tab, 48, seed=1, drop_last=True), sn.DeviceRayLoader(vtab, 48, seed=2)
    tool = sn.T_NeRF_Net_Tool(_args(12, n_saves=3, use_mse=True), hm, hm, "cuda", H4, WC, train_loader=train, val_loader=val, use_graph=True)
    assert tool.solar_vecs is train.solar_vecs and tool.solar_vecs.shape == (500, 3)
    tool.network.load_state_dict(orc.init_weights(64, 4, 1))
    np.random.seed(3); torch.manual_seed(3)
    graphed, colour = [], []
    for _ in range(12):
        tool.step()
        graphed.append(tool._graphed is not None and tool._graphed.graph is not None)
        colour.append(float(tool.last_loss["Color"][0]))
    assert graphed == [False] * 4 + [True] * 8
    assert tool._graphed.loader is train and train.get_state() == (1, 2, 12) and val.get_state()[2] == 2
    assert all(np.isfinite(colour)) and len(set(colour)) == 12          # twelve different batches
    short = sn.DeviceRayLoader(tab, 48, seed=1)                # 500 = 10 x 48 + 20: the eager path, and eligible() says why
    assert "drop_last" in sn.GraphedTrainStep.eligible(tool, short)
    bare = sn.T_NeRF_Net_Tool(_args(12, n_saves=3), hm, hm, "cuda", H4, WC)
    with pytest.raises(NotImplementedError):
        bare.get_data()
    with pytest.raises(NotImplementedError):
        sn.T_NeRF_Net_Tool(_args(12, n_saves=3), hm, hm, "cuda", H4, WC, train_loader=train).get_data(eval_mode=True)
    calls = []
    both = sn.T_NeRF_Net_Tool(_args(12, n_saves=3), hm, hm, "cuda", H4, WC, train_loader=train, get_data=lambda eval_mode: calls.append(eval_mode) or "mine")
    assert both.get_data() == "mine" and calls == [False]      # a callable still wins
