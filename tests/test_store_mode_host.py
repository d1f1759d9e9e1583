"""CPU: ERC_STEP_STORES is parsed strictly, and the header declares the switch the bindings are derived from."""
import ctypes as C

import pytest

from erc_amd import capi, engine


def test_step_stores_default_and_values(monkeypatch):
    monkeypatch.delenv("ERC_STEP_STORES", raising=False)
    assert engine.step_store_mode() == "through"
    monkeypatch.setenv("ERC_STEP_STORES", "")
    assert engine.step_store_mode() == "through"
    for mode in ("plain", "through"):
        monkeypatch.setenv("ERC_STEP_STORES", mode)
        assert engine.step_store_mode() == mode


@pytest.mark.parametrize("bad", ["Through", "wt", "0", "plain ", "sc1"])
def test_step_stores_rejects_unknown_values(monkeypatch, bad):
    monkeypatch.setenv("ERC_STEP_STORES", bad)
    with pytest.raises(capi.ErcGraftError, match="ERC_STEP_STORES"):
        engine.step_store_mode()


def test_header_declares_the_switch_and_the_library_exports_it():
    assert "erc_set_store_mode" in capi.EXPORTS
    res, args, names = capi.PROTOS["erc_set_store_mode"]
    assert (res, args, names) == (C.c_int, [C.c_int], ("mode",))
    capi.build()
    lib = capi.lib()
    assert lib.erc_set_store_mode(7) != 0 and b"set_store_mode" in lib.erc_last_error()      # refused before anything is launched
    assert lib.erc_set_store_mode(0) == 0 and lib.erc_set_store_mode(1) == 0
