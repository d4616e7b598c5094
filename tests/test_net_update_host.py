"""The in-place update entry points (include/az.h az_net_update*, az_net_generation, az_net_get_weights,
az_net_packed_read) refuse NULL handles with an error and a message, before they touch a device."""
import numpy as np
import pytest

import azchess._lib as L


def calls():
    w = np.zeros(8, np.float32)
    return {
        "az_net_update_device": lambda: L.lib.az_net_update_device(None, None, 8, None),
        "az_net_update": lambda: L.lib.az_net_update(None, L.fptr(w), w.size),
        "az_net_update_from_trainer": lambda: L.lib.az_net_update_from_trainer(None, None),
        "az_net_generation": lambda: L.lib.az_net_generation(None),
        "az_net_get_weights": lambda: L.lib.az_net_get_weights(None, L.fptr(w), w.size),
        "az_net_packed_read": lambda: L.lib.az_net_packed_read(None, 0, 0, None, 0),
    }


@pytest.mark.parametrize("name", sorted(calls()))
def test_null_handle_is_an_error_with_a_message(name):
    assert calls()[name]() < 0
    msg = L.lib.az_last_error().decode()
    assert name in msg and "null" in msg, msg
    with pytest.raises(L.AzError, match=name):
        L.check(calls()[name]())


def test_packed_kinds_match_the_header():
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "az.h")).read()
    enum = dict((k.lower(), int(v)) for k, v in re.findall(r"AZ_PACKED_([A-Z0-9_]+)\s*=\s*(\d+)", src))
    assert enum.pop("kinds") == len(L.PACKED_KINDS)
    assert enum == {k: i for i, k in enumerate(L.PACKED_KINDS)}
