"""Sharp evaluator families for the search tests (tests/test_sharpcases.py, tests/test_gpu_sharp_search.py).
TEST INFRASTRUCTURE ONLY.  numpy + oracle; nothing of the product is imported here.

A trained network gives one-hot priors, values at +-1 and, when it diverges, non-finite rows.  The synthetic
evaluator and random-initialised nets give none of these: their priors are near 1 / n, and a search tree
under them stays 4 to 5 plies deep.  Each family below is a pure function of a position's FEN key and its
distinct legal move indices in first-appearance order,

    family(key, idx) -> (row [4096] f32, value f32),

so the numpy restatements, the C oracle (through an O.Replay of the rows asked for) and the engine's
callback evaluator all see the same bits.  Entries of `row` that are not legal hold garbage (7.0, or NaN in
nanmix and allnan): the engine must read a row at the legal indices only."""
import numpy as np

import oracle as O

F = np.float32
M64 = (1 << 64) - 1
GRID5 = (-1.0, -0.5, 0.0, 0.5, 1.0)
GRID3 = (-1.0, 0.0, 1.0)
PHI = 0x9E3779B97F4A7C15
SALT_POS, SALT_NAN = 0x5A17C0DE5A17C0DE, 0x0DDBA11C0FFEE123


def splitmix64(x):
    x = (x + PHI) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _edge_hash(key, i, salt=0):
    return splitmix64(key ^ salt ^ (((int(i) + 1) * PHI) & M64))


def _row(idx, fill=7.0):
    row = np.full(4096, fill, F)
    row[idx] = F(0.0)
    return row


def first(key, idx):
    """prior 1 on the first legal move, 0 elsewhere, value 0"""
    row = _row(idx)
    row[idx[0]] = F(1.0)
    return row, F(0.0)


def last(key, idx):
    """prior 1 on the last legal move, 0 elsewhere, value 0"""
    row = _row(idx)
    row[idx[-1]] = F(1.0)
    return row, F(0.0)


def hashed(key, idx):
    """prior 1 on one hashed legal move, 0 elsewhere; value -1, 0 or +1 by hash"""
    h = splitmix64(key ^ SALT_POS)
    row = _row(idx)
    row[idx[h % len(idx)]] = F(1.0)
    return row, F(GRID3[(h >> 20) % 3])


def zeros(key, idx):
    """every legal prior 0: the selection runs on q alone; value on the 5-point grid by hash"""
    h = splitmix64(key ^ SALT_POS)
    return _row(idx), F(GRID5[(h >> 20) % 5])


def uniform(key, idx):
    """every legal prior f32(1) / f32(n), value 0: every selection is an exact n-way tie"""
    row = _row(idx)
    row[idx] = F(1.0) / F(len(idx))
    return row, F(0.0)


def tiny(key, idx):
    """hashed integer weights 1..256 times 2^-140: every prior an f32 subnormal; value 0"""
    row = _row(idx)
    for i in idx:
        row[i] = F(np.ldexp(float(1 + (_edge_hash(key, i) >> 56)), -140))
    return row, F(0.0)


def nanmix(key, idx):
    """the synthetic evaluator's priors with about 1/8 of the legal entries NaN (never the first) and about
    1/8 +inf; value NaN on about a quarter of the positions, else the 5-point grid; non-legal entries NaN"""
    h = splitmix64(key ^ SALT_POS)
    row = _row(idx, np.nan)
    w = [1 + (_edge_hash(key, i) >> 48) for i in idx]
    row[idx] = np.array(w, F) / F(sum(w))
    for k, i in enumerate(idx):
        r = _edge_hash(key, i, SALT_NAN) % 8
        if r == 0 and k > 0:
            row[i] = F(np.nan)
        elif r == 1:
            row[i] = F(np.inf)
    return row, (F(np.nan) if (h >> 20) % 4 == 0 else F(GRID5[(h >> 22) % 5]))


def allnan(key, idx):
    """a diverged network: every entry and the value NaN"""
    return np.full(4096, np.nan, F), F(np.nan)


FAMILIES = dict(first=first, last=last, hashed=hashed, zeros=zeros, uniform=uniform, tiny=tiny, nanmix=nanmix,
                allnan=allnan)


def distinct(indices):
    """the distinct legal indices in first-appearance order (under-promotions share an index)"""
    return list(dict.fromkeys(int(i) for i in indices))


def ref_evaluator(family, log=None):
    """the family as an evaluator of the references: RefPos -> (row, value).  log (a dict): receives
    key -> (idx, row, value) of every position asked for (see replay_of)."""
    fn = FAMILIES[family] if isinstance(family, str) else family

    def ev(pos):
        key, idx = int(O.fen_key(pos)), distinct(O.legal_indices(pos))
        row, val = fn(key, idx)
        if log is not None:
            log[key] = (idx, row, val)
        return row, val
    return ev


def gpu_evaluator(family, calls=None):
    """the family as a callback evaluator of the engine: [Position] -> (pol [n, 4096], val [n])"""
    fn = FAMILIES[family] if isinstance(family, str) else family

    def ev(states):
        if calls is not None:
            calls.append(len(states))
        pol = np.empty((len(states), 4096), F)
        val = np.empty(len(states), F)
        for r, p in enumerate(states):
            pol[r], val[r] = fn(int(p.fen_key()), distinct(p.legal_indices()))
        return pol, val
    return ev


def replay_of(log):
    """an O.Replay (the C oracle's evaluator) of the rows a ref_evaluator logged"""
    keys, vals, off, idx, pri = [], [], [0], [], []
    for key, (ix, row, val) in log.items():
        keys.append(key)
        vals.append(val)
        idx += ix
        pri += [row[i] for i in ix]
        off.append(len(idx))
    return O.Replay(np.array(keys, np.uint64), np.array(vals, F), np.array(off, np.int32), np.array(idx, np.int32),
                    np.array(pri, F))
