"""CPU: capi.py takes every ctypes type from include/ercgraft.h, and _call checks a wrapper's arguments against the
prototype before anything reaches the library or the GPU."""
import ctypes as C
import os
import re

import pytest
import torch

from erc_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SAMPLE = r'''
#ifndef SAMPLE_H
#define SAMPLE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define ERC_ABI_VERSION 7
int erc_abi_version(void);
const char* erc_last_error(void);
/* int erc_commented_out(int a, void* stream); */
typedef struct ErcThing {
    int64_t a, b;   // erc_not_a_prototype(int x);
    int32_t c;
} ErcThing;
int erc_multi(const float* A, int lda,
              int64_t n, /* a comment: int erc_inner(float x); */ uint64_t seed,
              float scale, const ErcThing* thing_host,
              int32_t* out, void* stream);
int64_t erc_ws_floats(int n_rows);
int erc_set(const int32_t * const t);
#ifdef __cplusplus
}
#endif
#endif
'''


def test_parse_header_types_names_and_layout():
    p = capi.parse_header(SAMPLE)
    assert set(p) == {"erc_abi_version", "erc_last_error", "erc_multi", "erc_ws_floats", "erc_set"}
    assert p["erc_abi_version"] == (C.c_int, [], ())
    assert p["erc_last_error"] == (C.c_char_p, [], ())
    assert p["erc_multi"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_void_p, C.c_void_p,
                                        C.c_void_p],
                              ("A", "lda", "n", "seed", "scale", "thing_host", "out", "stream"))
    assert p["erc_ws_floats"] == (C.c_int64, [C.c_int], ("n_rows",))
    assert p["erc_set"] == (C.c_int, [C.c_void_p], ("t",))


@pytest.mark.parametrize("decl", ["int erc_bad(double x, void* stream);", "int erc_bad(size_t n);", "void erc_bad(int n);",
                                  "int erc_bad(int);", "int erc_bad();"])
def test_parse_header_refuses_what_it_cannot_map(decl):
    with pytest.raises(capi.ErcGraftError, match="erc_bad"):
        capi.parse_header(decl)


def test_real_header_binds_every_declaration():
    header = open(os.path.join(REPO, "include", "ercgraft.h")).read()
    assert capi.ERC_ABI_VERSION == int(re.search(r"#define ERC_ABI_VERSION (\d+)", header).group(1))
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = dict(re.findall(r"\b(erc_[a-z0-9_]+)\s*\(([^()]*)\)", bare))
    assert set(decls) == set(capi.EXPORTS) == set(capi.PROTOS)
    n_launching = 0
    for name, (res, argtypes, names) in capi.PROTOS.items():
        n_params = 0 if decls[name].strip() == "void" else decls[name].count(",") + 1
        assert len(argtypes) == len(names) == n_params, name
        launches = re.search(r"void\s*\*\s*stream\s*$", decls[name]) is not None
        assert capi._launches(name) == launches, name
        assert "stream" not in names[:-1], name
        n_launching += launches
        assert res in (C.c_int, C.c_int64) or name == "erc_last_error", name
    assert 0 < n_launching < len(capi.PROTOS)


def test_call_checks_the_argument_count():
    n = len(capi.PROTOS["erc_slab_reduce"][2]) - 1          # stream excluded
    with pytest.raises(capi.ErcGraftError, match="erc_slab_reduce"):
        capi._call("erc_slab_reduce", *([None] * (n + 1)))
    with pytest.raises(capi.ErcGraftError, match="erc_slab_reduce"):
        capi._call("erc_slab_reduce", *([None] * (n - 1)))
    with pytest.raises(capi.ErcGraftError, match="erc_wgrad_bf16_set_spin_limit"):
        capi._call("erc_wgrad_bf16_set_spin_limit", 1, 2)   # no stream: all parameters are the caller's


def test_call_refuses_host_tensors_for_device_operands():
    x = torch.zeros(16)
    with pytest.raises(capi.ErcGraftError, match=r"erc_slab_reduce: slabs .*cpu"):
        capi._call("erc_slab_reduce", x, 1, 0, None, 16, 0, None, 0, 16)
    with pytest.raises(capi.ErcGraftError, match=r"erc_gemm_x3: C .*cpu"):
        capi.gemm_x3(None, 4, None, 4, x, 4, 4, 4, 4)
