"""Compiles and runs tests/cpp/test_hash_api.cpp — the C++ host-side mirror (include/poseidon252.hpp)
of the reference's Hash/Domain API over the C ABI — on the GPU."""
import pytest

from helpers.percall import build_cpp_mirror, run_cpp_mirror


def _build(tmp_path):
    return build_cpp_mirror("test_hash_api", tmp_path, flags=(), hip_runtime=True)


def test_cpp_mirror_compiles(tmp_path, oracle_mod):
    """(CPU) the header-only mirror compiles and links against the C ABI"""
    _build(tmp_path)


@pytest.mark.gpu
def test_cpp_mirror_on_gpu(tmp_path, oracle_mod, gpu_ctx):
    exe = _build(tmp_path)
    assert "ALL PASSED" in run_cpp_mirror(exe)
