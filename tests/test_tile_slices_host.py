"""CPU: ERC_TILE_SLICES is parsed strictly, and the header declares the switch and the node_rec argument the bindings are derived from."""
import ctypes as C

import pytest

from erc_amd import capi, engine


def test_tile_slices_default_and_values(monkeypatch):
    monkeypatch.delenv("ERC_TILE_SLICES", raising=False)
    assert engine.tile_slice_mode() == "closed"
    monkeypatch.setenv("ERC_TILE_SLICES", "")
    assert engine.tile_slice_mode() == "closed"
    for mode in ("csr", "closed"):
        monkeypatch.setenv("ERC_TILE_SLICES", mode)
        assert engine.tile_slice_mode() == mode


@pytest.mark.parametrize("bad", ["Closed", "CSR", "1", "closed ", "records"])
def test_tile_slices_rejects_unknown_values(monkeypatch, bad):
    monkeypatch.setenv("ERC_TILE_SLICES", bad)
    with pytest.raises(capi.ErcGraftError, match="ERC_TILE_SLICES"):
        engine.tile_slice_mode()


def test_header_declares_the_switch_and_the_library_exports_it():
    assert "erc_set_tile_slices" in capi.EXPORTS
    res, args, names = capi.PROTOS["erc_set_tile_slices"]
    assert (res, args, names) == (C.c_int, [C.c_int], ("mode",))
    capi.build()
    lib = capi.lib()
    assert lib.erc_set_tile_slices(7) != 0 and b"set_tile_slices" in lib.erc_last_error()      # refused before anything is launched
    assert lib.erc_set_tile_slices(0) == 0 and lib.erc_set_tile_slices(1) == 0


TILE_ENTRY_POINTS = ("erc_cogmen_fwd_tile", "erc_cogmen_fwd_tile_x", "erc_cogmen_bwd_tile", "erc_cogmen_bwd_tile_x",
                     "erc_cogmen_project_graph", "erc_cogmen_project_graph_x")


@pytest.mark.parametrize("name", TILE_ENTRY_POINTS)
def test_header_and_bindings_agree_on_node_rec(name):
    """node_rec is the last argument in front of the stream, a pointer: the derived prototype has it where the header does"""
    res, args, names = capi.PROTOS[name]
    assert res == C.c_int and len(args) == len(names)
    assert names[-2:] == ("node_rec", "stream") and names.count("node_rec") == 1
    assert args[-2] == C.c_void_p and args[-1] == C.c_void_p
    want = {"erc_cogmen_fwd_tile": "events", "erc_cogmen_fwd_tile_x": "events", "erc_cogmen_bwd_tile": "n_dev",
            "erc_cogmen_bwd_tile_x": "n_dev", "erc_cogmen_project_graph": "desc", "erc_cogmen_project_graph_x": "desc"}[name]
    assert names[-3] == want
    capi.build()
    capi.lib()
    assert list(getattr(capi._raw, name).argtypes) == list(args)
