"""The entry points that carry self-play games across a weight update (az_selfplay_adopt_net,
az_search_adopt_net, az_selfplay_inflight), without a GPU: they are exported with the declared
signatures, refuse a NULL handle with a message, and train(carry_games=True) refuses more than one
rank before anything touches a device."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

I32P = C.POINTER(C.c_int32)
WANT = {
    "az_selfplay_adopt_net": ("int", ["az_search*"], [C.c_void_p]),
    "az_search_adopt_net": ("int", ["az_search*", "int"], [C.c_void_p, C.c_int]),
    "az_selfplay_inflight": ("int", ["az_search*", "int32_t*", "int32_t*", "int32_t*", "int32_t*", "int32_t*", "int"],
                             [C.c_void_p, I32P, I32P, I32P, I32P, I32P, C.c_int]),
}


def declarations():
    """{name: (return type, [parameter types])} of include/az.h, comments stripped"""
    src = open(os.path.join(ROOT, "include", "az.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b([a-z0-9_]+\s*\**)\s*\b(az_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        params = [re.sub(r"\s*\b[a-z_0-9]+$", "", a.strip()).replace(" ", "") for a in args.split(",")]
        out[name] = (ret.replace(" ", ""), params)
    return out


def test_header_and_binding_declare_the_signatures():
    import azchess._lib as L
    decl = declarations()
    bound = {n: (r, a) for n, r, a in L.SIGNATURES}
    for name, (ret, params, ctypes_args) in WANT.items():
        assert decl[name] == (ret, params), name
        assert bound[name] == (C.c_int, ctypes_args), name
        assert hasattr(C.CDLL(L.LIB_PATH), name), name


def test_null_handle_is_an_error_with_a_message():
    import azchess._lib as L
    calls = {"az_selfplay_adopt_net": lambda: L.lib.az_selfplay_adopt_net(None),
             "az_search_adopt_net": lambda: L.lib.az_search_adopt_net(None, 1),
             "az_selfplay_inflight": lambda: L.lib.az_selfplay_inflight(None, None, None, None, None, None, 0)}
    assert set(calls) == set(WANT)
    for name, call in calls.items():
        L.lib.az_version()
        assert call() < 0, name
        assert L.lib.az_last_error().decode() == "null search", name


def test_train_carry_games_refuses_more_than_one_rank():
    """before any device call: this machine may have no GPU, and the reducer is never installed"""
    import azchess as A

    def reduce(buf):
        raise AssertionError("the reducer ran")

    with pytest.raises(ValueError, match="^carry_games: one rank for now$"):
        A.train(1, carry_games=True, reducer=(reduce, 0, 2))
