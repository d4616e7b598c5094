"""The host side of train()'s model gate (training.rs:131-132, 208-232): the verdict in float32, the
match's seed, the verdict's exchange between ranks, and the new trainer entry points refusing a null
handle without touching a device."""
import ctypes as C

import pytest

import azchess as A
import azchess._lib as L
from azchess.training import agree_verdict, elo_seed, gate_seed, gate_verdict, sample_seed

NEW_SYMBOLS = ["az_trainer_set_params", "az_trainer_set_params_device", "az_trainer_snapshot", "az_trainer_restore",
               "az_trainer_get_snapshot", "az_trainer_adamw_steps"]


def test_parameters():
    assert A.parameters.SKIP_VALIDATION is True
    assert A.parameters.WIN_RATE_THRESHOLD == 0.55
    assert A.gate_verdict is gate_verdict and A.gate_seed is gate_seed and A.agree_verdict is agree_verdict


@pytest.mark.parametrize("winrate,threshold,want", [
    (281 / 512, 0.55, False),     # 0.548828125
    (282 / 512, 0.55, True),      # 0.55078125
    (0.55, 0.55, True),           # the double 0.55 against the f32 0.55: equal once both are f32
    (0.0, 0.0, True),
    (1.0, 1.5, False),
])
def test_gate_verdict_compares_in_float32(winrate, threshold, want):
    assert gate_verdict(winrate, threshold) is want


def test_gate_seed_is_its_own():
    for seed in (0, 5, 42):
        for it in (0, 1, 255, 256):
            g = gate_seed(seed, it)
            assert g != elo_seed(seed, it)
            assert all(g != sample_seed(seed, it, step) for step in range(64))
            assert all(g != sample_seed(seed, it, step, rank) for step in range(64) for rank in range(8))


def _fake_allgather(verdicts):
    """allgather for rank r of an in-process world whose other ranks pass verdicts[...]."""
    def ag(rank):
        def gather(payload):
            assert isinstance(payload, bytes) and len(payload) == 1
            out = [b"\x01" if v else b"\x00" for v in verdicts]
            assert out[rank] == payload
            return out
        return gather
    return ag


@pytest.mark.parametrize("v", [True, False])
def test_agree_verdict_equal(v):
    ag = _fake_allgather([v, v])
    assert agree_verdict(v, ag(0)) == (v, True)
    assert agree_verdict(v, ag(1)) == (v, True)


def test_agree_verdict_takes_rank_zeros():
    ag = _fake_allgather([True, False])
    assert agree_verdict(True, ag(0)) == (True, False)
    assert agree_verdict(False, ag(1)) == (True, False)
    ag = _fake_allgather([False, True, True])
    assert agree_verdict(True, ag(2)) == (False, False)


def test_new_symbols_are_bound():
    bound = {n for n, _, _ in L.SIGNATURES}
    assert set(NEW_SYMBOLS) <= bound


def test_null_trainer_fails_without_a_device():
    w = (C.c_float * 4)()
    calls = {
        "az_trainer_snapshot": lambda: L.lib.az_trainer_snapshot(None),
        "az_trainer_restore": lambda: L.lib.az_trainer_restore(None),
        "az_trainer_set_params": lambda: L.lib.az_trainer_set_params(None, w, 4),
        "az_trainer_set_params_device": lambda: L.lib.az_trainer_set_params_device(None, None, 4, None),
        "az_trainer_get_snapshot": lambda: L.lib.az_trainer_get_snapshot(None, w, 4),
        "az_trainer_adamw_steps": lambda: L.lib.az_trainer_adamw_steps(None),
    }
    for name, call in calls.items():
        assert call() < 0, name
        err = L.lib.az_last_error()
        err = err.decode() if isinstance(err, bytes) else str(err)
        assert err and name in err, (name, err)


def test_train_gate_needs_an_allgather_at_world_2():
    """Gate on at world > 1 with no way to exchange the verdicts: refused on the host, before a trainer
    touches a GPU."""
    red = (lambda buf: None, 0, 2)
    with pytest.raises(ValueError, match="allgather"):
        A.train(1, reducer=red, gate=True, shared_replay=False, shard_batch=False)
