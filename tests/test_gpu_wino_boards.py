"""tower32w2_kernel: the 256-filter row-direct shared-row tower with two batch rows per workgroup on one
weight stream and the residual convs' activations in global memory (wino.h wino_core_b2, AZ_WINO_BOARDS=2)
against the one-board kernel (AZ_WINO_BOARDS=1).  Per board the products, their order and K are the same, so
every output is bit-equal; and against the oracle, the float64 reference and the f32-product kernel as the
shared-row test.  Every test asserts which form ran (AlphaZero.wino_boards)."""
import numpy as np
import pytest

import azchess as A
import azchess._lib as L
import netcases as N
import oracle as O
from test_gpu_net import check, random_planes
from test_gpu_wino_derive import PLAIN, SPLIT
from test_gpu_wino_rows import tower_inputs64
from test_netcases import get_case
from test_wino_derive import exact_planes, exact_weights

pytestmark = pytest.mark.gpu

BOARDS_DEFAULT = 2     # az_internal.h AZ_WINO_BOARDS_DEFAULT
# 1. f3 e5 2. g4: Black to move mates with Qh4, a terminal leaf (no network row) whenever it is selected
MATE_IN_ONE = ["rnbqkbnr/pppppppp/8/8/8/5P2/PPPPP1PP/RNBQKBNR", "rnbqkbnr/pppp1ppp/8/4p3/8/5P2/PPPPP1PP/RNBQKBNR",
               "rnbqkbnr/pppp1ppp/8/4p3/6P1/5P2/PPPPP2P/RNBQKBNR"]


def net_at(monkeypatch, boards, blocks, w, filters=256, **other):
    """a f32 net created with AZ_WINO_BOARDS=boards and AZ_WINO_VROWS / ROWS / DERIVE / SPLIT16 from `other`
    (None: unset); the form it reports is asserted"""
    env = dict(AZ_WINO_BOARDS=boards, AZ_WINO_VROWS=other.get("vrows"), AZ_WINO_ROWS=other.get("rows"),
               AZ_WINO_DERIVE=other.get("derive"), AZ_WINO_SPLIT16=other.get("split16"))
    for name, v in env.items():
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    net = A.AlphaZero(blocks, filters, weights=w, dtype="f32")
    shared = filters == 256 and all(other.get(k) in (None, 1) for k in ("vrows", "rows", "derive", "split16"))
    if shared:
        want = BOARDS_DEFAULT if boards is None else (2 if boards == 2 else 1)
        assert net.tower_kernel == SPLIT and net.wino_v_rows == 1 and net.wino_boards == want
    elif other.get("split16") == 0:
        assert net.tower_kernel == PLAIN and net.wino_boards == 0
    else:
        assert "split-f16 MFMA" in net.tower_kernel and net.wino_v_rows == 0 and net.wino_boards == 1
    return net


def both(monkeypatch, blocks, w, planes):
    """forward with the knob at 2 and at 1; asserts bit-equality and returns the outputs at 2"""
    p2, v2 = net_at(monkeypatch, 2, blocks, w).forward(planes)
    p1, v1 = net_at(monkeypatch, 1, blocks, w).forward(planes)
    assert np.array_equal(v2, v1, equal_nan=True), np.abs(v2 - v1).max()
    assert np.array_equal(p2, p1, equal_nan=True), np.abs(p2 - p1).max()
    return p2, v2


def test_knob_and_accessor(require_gpu, monkeypatch):
    """unset follows the compiled default; 1 and 2 report 1 and 2, any other value 1; every other form reports
    one board (0 without the split-f16 tower) whatever the knob says, and evaluates as with the knob unset"""
    w = A.random_weights(1, 256, seed=3)
    planes = random_planes(3, 13)
    for boards in (None, 1, 2, 3):
        net_at(monkeypatch, boards, 1, w)
    for other in (dict(vrows=0), dict(rows=0), dict(derive=0), dict(split16=0)):
        want = net_at(monkeypatch, None, 1, w, **other).forward(planes)
        got = net_at(monkeypatch, 2, 1, w, **other).forward(planes)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), other
    for filters in (128, 64):
        net_at(monkeypatch, 2, 1, A.random_weights(1, filters, seed=3), filters=filters, split16=2)


@pytest.mark.parametrize("blocks", [1, 2, 3])
def test_dense_bit_equal(require_gpu, monkeypatch, blocks):
    """rows 1, 2, 3, 5: a lone board, a full pair, an odd tail behind one and behind two full pairs"""
    w = A.random_weights(blocks, 256, seed=3 + blocks)
    planes = random_planes(5, 13 + blocks)
    n2, n1 = net_at(monkeypatch, 2, blocks, w), net_at(monkeypatch, 1, blocks, w)
    for rows in (1, 2, 3, 5):
        (p2, v2), (p1, v1) = n2.forward(planes[5 - rows:]), n1.forward(planes[5 - rows:])
        assert np.array_equal(p2, p1) and np.array_equal(v2, v1), rows
        assert np.isfinite(p2).all() and np.all(np.abs(p2.astype(np.float64).sum(1) - 1.0) <= 1e-6)


def run_search(net, hist, sims, start=None, **kw):
    s = A.BatchedSearch(net, games=len(hist), sims=sims, seed=3, **kw)
    s.set_roots(hist, apply_noise=True)
    imp, vis, dep = s.run()
    return np.array(imp), np.array(vis), np.array(dep), s


@pytest.mark.parametrize("games", [1, 2, 3, 5])
@pytest.mark.parametrize("blocks", [1, 2, 3])
def test_search_bit_equal(require_gpu, monkeypatch, blocks, games):
    """a 16-simulation search through k_step + the tower, knob at 2 against 1: bit-equal visits and improved
    policies.  The persistent kernel stays on one board and gives the same search"""
    w = A.random_weights(blocks, 256, seed=42)
    hist = [[], [588], [], [588], []][:games]
    got = []
    for boards in (2, 1):
        net = net_at(monkeypatch, boards, blocks, w)
        imp, vis, dep, s = run_search(net, hist, 16)
        assert not s.persistent
        got.append((imp, vis, dep))
    imp, vis, dep, s = run_search(net_at(monkeypatch, 2, blocks, w), hist, 16, cache_capacity=0)
    assert s.persistent
    got.append((imp, vis, dep))
    assert got[0][1].sum() > 0
    for g in got[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(g, got[0]))


def mate_history():
    """move indices of 1. f3 e5 2. g4, found by their resulting positions"""
    p, hist = A.Position.startpos(), []
    for board in MATE_IN_ONE:
        nxt = [i for i in p.legal_indices() if p.play(i).fen().split()[0] == board]
        assert len(nxt) == 1, board
        hist.append(int(nxt[0]))
        p = p.play(nxt[0])
    return hist


def test_search_count_cuts_a_pair(require_gpu, monkeypatch):
    """A device count below rows that cuts a pair in half.  Evaluation cache off and the persistent kernel off
    (AZ_PERSIST=0), so every game either sends one row to the tower or reaches a terminal leaf in every
    simulation step.  The quiet games reach none and send a row in every step (asserted on their own; they are
    the same games with the same seeds in the full search), so every step in which the mate game selects the
    mate (a terminal leaf, or an edge already known to win) launches the tower with count = rows - 1: 1 of 2 (the pair of
    workgroup 0 cut in half), 3 of 4 (the pair of workgroup 1 cut in half) and 2 of 3 (workgroup 1 absent).
    Nothing is written for a row at or beyond count: the evaluation log, to which the heads add one record per
    row they write out, holds exactly the rows counted and the roots (an absent row that ran its heads would add one, and
    its stale row -> node map points at a node evaluated earlier, whose priors it would overwrite); visits,
    improved policies and the log are bit-equal to the one-board kernel's.  (The value and prior buffers
    of a search cannot be poisoned or read through the API.)"""
    monkeypatch.setenv("AZ_PERSIST", "0")
    w = A.random_weights(2, 256, seed=42)
    mate = mate_history()
    kw = dict(cache_capacity=0, record_evals=True, eval_log_cap=8192)
    sims = 96
    for hist in ([[], mate], [[], [588], [], mate], [[], [588], mate]):
        got = []
        for boards in (2, 1):
            net = net_at(monkeypatch, boards, 2, w)
            *_, quiet = run_search(net, hist[:-1], sims, **kw)
            assert not quiet.persistent and quiet.stats()["terminal_leaves"] == 0
            imp, vis, dep, s = run_search(net, hist, sims, **kw)
            st = s.stats()
            T = st["terminal_leaves"]
            keys, vals, off, idx, pri = s.eval_log()
            per_game = quiet.stats()["evals"] // (len(hist) - 1)      # rows of a game that reaches no terminal leaf
            print("games %d boards %d: %d terminal leaves, %d rows, %d logged, %d per quiet game"
                  % (len(hist), boards, T, st["evals"], len(keys), per_game))
            assert not s.persistent and T > 0
            # the quiet games send a row in every simulation step; the mate game's rows are the rest, and in every
            # step without one the count was rows - 1
            assert per_game == sims and quiet.stats()["evals"] == per_game * (len(hist) - 1)
            cut = per_game - (st["evals"] - quiet.stats()["evals"])
            print("steps with count = rows - 1: %d" % cut)
            assert 0 < cut <= per_game
            # one record per row written out -- the simulation steps' rows and one root evaluation per game (set_roots,
            # before the counters start: the quiet search shows the same accounting) -- and none for an absent row
            assert len(quiet.eval_log()[0]) == quiet.stats()["evals"] + len(hist) - 1
            assert len(keys) == st["evals"] + len(hist)
            got.append((imp, vis, dep, np.sort(keys), T, st["evals"]))
        assert all(np.array_equal(a, b) for a, b in zip(got[0], got[1]))


def test_random_weights_against_oracle(require_gpu, monkeypatch):
    w = A.random_weights(2, 256, seed=3)
    planes = random_planes(3, 13)
    pol, val = both(monkeypatch, 2, w, planes)
    rpol, rval = O.RefNet(2, 256, w).forward(planes)
    check(pol, val, rpol, rval, "f32")


@pytest.mark.parametrize("family", ["gamma5", "signed"])
def test_trained_like_weights(require_gpu, monkeypatch, family):
    """channel spread 2^+-5 / negative gamma (tests/netcases.py): bit-equal to one board per workgroup, within
    the project's tolerance of float64 and within M = 8 times the plain float32 evaluation's own error"""
    c = get_case(family, 2, 256, 5)
    pol, val = both(monkeypatch, 2, c.w, c.planes)
    ratios = N.measured_bound(pol, val, c, "f32-split16 rows, two boards", enforce=False)
    N.check_tolerance(pol, val, c, "f32")
    N.assert_measured(ratios, c)


def test_exact_arithmetic(require_gpu, monkeypatch):
    """weights and planes on which every product and sum is exact: bit-equal to the one-board kernel and to
    the f32-product kernel"""
    w = exact_weights(2, 256, 1)
    planes = exact_planes(4, 2)
    pol, val = both(monkeypatch, 2, w, planes)
    fpol, fval = net_at(monkeypatch, None, 2, w, split16=0).forward(planes)
    assert np.array_equal(pol, fpol) and np.array_equal(val, fval)
    rpol, rval = N.forward64(2, 256, w, planes)
    check(pol, val, rpol, rval, "f32")
    assert np.unique(val).size == 4 and pol.max() > 2.0 / 4096     # not a dead net


def test_20_blocks(require_gpu, monkeypatch):
    """the ring, the zero rows, the hand-off and the global activations carried over 40 conv boundaries"""
    pol, val = both(monkeypatch, 20, A.random_weights(20, 256, seed=42), random_planes(3, 20256))
    assert np.isfinite(pol).all() and np.isfinite(val).all()


def test_partner_is_not_contaminated(require_gpu, monkeypatch):
    """one board of a pair with its planes scaled up 2^16 x (the layer inputs of the rows test's overflow case)
    leaves the f16 range and comes out NaN; its partner's outputs are those it has beside an ordinary board,
    in either seat of the pair"""
    w = A.random_weights(2, 256, seed=3)
    net = net_at(monkeypatch, 2, 2, w)
    a, b, c = random_planes(3, 13)
    # the planes are scaled (the weights are the pair's): by as much as puts the first residual conv's largest
    # input, computed in float64, where the overflow case has it -- 2^16 x the ordinary board's
    peak = lambda x: float(tower_inputs64(2, w, x[None])[0].max())
    slope = peak(a * np.float32(65536.0)) / 65536.0               # the peak per unit of plane scale, far above the bias
    big = a * np.float32(65536.0 * peak(b) / slope)
    print("first residual conv's largest input: big board %.3g, partner %.3g" % (peak(big), peak(b)))
    assert peak(big) > 0.99 * 65536.0 * peak(b) > 65504.0 / 128 and peak(b) < 255
    for seat in (0, 1):
        pair = lambda other: np.stack([b, other] if seat else [other, b])
        pol, val = net.forward(pair(big))
        wpol, wval = net.forward(pair(c))
        assert not np.isfinite(pol[seat]).any() and not np.isfinite(val[seat])
        assert np.isfinite(pol[1 - seat]).all()
        assert np.array_equal(pol[1 - seat], wpol[1 - seat]) and val[1 - seat] == wval[1 - seat]


def test_two_streams_back_to_back(require_gpu, monkeypatch):
    """two forwards of one net on two streams with nothing between them (the global activations are kept per
    stream): each gives its single-stream result.  Both carry the same rows: az_net_forward_device stages its
    planes in a buffer of the net's, which two streams may only fill with the same bytes; the towers' global
    activations would still collide, the two launches being at different convs at any one time"""
    from azchess.hiprt import Hip
    hip = Hip()
    net = net_at(monkeypatch, 2, 8, A.random_weights(8, 256, seed=7))
    x = np.ascontiguousarray(random_planes(4, 31).reshape(4, -1))
    xs = [x, x]
    want = [net.forward(x) for x in xs]
    streams = [hip.stream(), hip.stream()]
    bufs = [(hip.malloc(x.nbytes), hip.malloc(len(x) * 4096 * 4), hip.malloc(len(x) * 4)) for x in xs]
    try:
        for rep in range(2):
            for x, (d_in, d_pol, d_val) in zip(xs, bufs):
                hip.copy_in(d_in, x)
                hip.copy_in(d_pol, np.full((len(x), 4096), np.nan, np.float32))
                hip.copy_in(d_val, np.full(len(x), np.nan, np.float32))
            for x, (d_in, d_pol, d_val), st in zip(xs, bufs, streams):
                L.check(L.lib.az_net_forward_device(net._h, d_in, len(x), d_pol, d_val, st))
            for st in streams:
                hip.stream_synchronize(st)
            for x, (d_in, d_pol, d_val), (wpol, wval) in zip(xs, bufs, want):
                pol = hip.download(d_pol, np.zeros((len(x), 4096), np.float32))
                val = hip.download(d_val, np.zeros(len(x), np.float32))
                assert np.array_equal(pol, wpol) and np.array_equal(val, wval), rep
    finally:
        for st in streams:
            hip.stream_destroy(st)
        for b in bufs:
            for p in b:
                hip.free(p)


def test_row_counts_grow_and_shrink(require_gpu, monkeypatch):
    """launches of 1, 5, 2 and 7 rows on one net (the global activations grow on demand): each bit-equal to
    the one-board kernel"""
    w = A.random_weights(2, 256, seed=9)
    n2, n1 = net_at(monkeypatch, 2, 2, w), net_at(monkeypatch, 1, 2, w)
    planes = random_planes(7, 44)
    for rows in (1, 5, 2, 7):
        (p2, v2), (p1, v1) = n2.forward(planes[:rows]), n1.forward(planes[:rows])
        assert np.array_equal(p2, p1) and np.array_equal(v2, v1), rows
