"""CPU: the chunk arithmetic of the cross-launch record sums (csrc/record_chunks.h: which records a wavefront of
head_fused_kernel<true, .> or cogmen_bwd_tile_kernel adds up) as a host program under the address and undefined-behaviour
sanitizers.  The GPU side is tests/test_gpu_record_sums.py."""
import os
import shutil
import subprocess

from erc_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_record_chunks_under_the_address_and_undefined_sanitizers(tmp_path):
    """tests/host/record_chunks_check.cpp walks the kernels' own load loop for 0 .. 600 records, 8 and 16 wavefronts and records
    of 50, 57 and 64 float4 over exactly sized heap buffers: every (record, slot) is covered once, the chunks are contiguous
    and ordered, nothing at or beyond the record count is dereferenced"""
    hipcc = os.path.realpath(os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc")
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin", "clang++")
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++, %s): the host memory check cannot run" % rocm_clang
    exe = str(tmp_path / "record_chunks_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", capi.CSRC, os.path.join(REPO, "tests", "host", "record_chunks_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.startswith("ok %d" % (601 * 2 * 3)), (res.stdout[-500:], res.stderr[-2000:])
