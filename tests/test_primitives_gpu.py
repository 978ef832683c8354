"""Every field primitive of csrc/fr29.hpp / hades29.hpp as the KERNELS compile it (csrc/primtest.hip: one kernel per primitive,
one case per lane), on the cases of tests/primcases.py: the documented contract checked in big integers, and the device's raw
output compared digit for digit with the host build's.  The arithmetic is integer and deterministic, so a difference between the
two is a divergence of the device path — twice() as inline v_add_u32, the ranges opaque_digit / make_rk hide from the optimiser
on the device only — and the message says so.  The output stage (store_output<false|true>) exists only in device code: it is
checked against big integers alone."""
import ctypes
import os

import numpy as np
import pytest

import primcases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def primtest_dev():
    import torch  # noqa: F401  (torch's HIP runtime is the one in the process before either library loads)
    import poseidon252_amd  # noqa: F401
    from poseidon252_amd import _lib, build as b
    _lib.lib()
    path = b.PRIMTEST_DEV_LIB if os.path.exists(b.PRIMTEST_DEV_LIB) else b.build_primtest_device()
    return ctypes.CDLL(path)


@pytest.fixture(scope="module")
def primtest_host():
    from poseidon252_amd import build as b
    return ctypes.CDLL(b.build_primtest_host())


@pytest.fixture(scope="module")
def table(hosttest_lib, primtest_host):
    return pc.load_table(hosttest_lib), pc.load_layout(primtest_host)


def run_device(lib, cs):
    """one launch over all cases of cs; returns the raw output rows"""
    import torch
    fn = getattr(lib, "ptd_" + cs.entry)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    n = len(cs)
    d_a = torch.from_numpy(cs.a_arr if cs.a_arr.size else np.zeros((1, 1), dtype=np.int32)).to("cuda:0").contiguous()
    d_b = torch.from_numpy(cs.b_arr if cs.b_arr.size else np.zeros((1, 1), dtype=np.int64)).to("cuda:0").contiguous()
    if cs.a_arr.size:
        assert d_a.numel() == n * cs.a_arr.shape[1]
    if cs.b_arr.size:
        assert d_b.numel() == n * cs.b_arr.shape[1]
    d_out = torch.full((n, pc.out_stride(cs)), 0x5a5a5a5a, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    rc = fn(d_a.data_ptr(), d_b.data_ptr(), d_out.data_ptr(), n)
    assert rc == 0, "%s: launch failed with hipError %d" % (cs.entry, rc)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("prim", pc.HOST_PRIMS)
def test_primitive_contract_on_device(prim, primtest_dev, primtest_host, table):
    tab, lay = table
    for cs in pc.cases_for(prim, tab, lay):
        got = run_device(primtest_dev, cs)
        worst = cs.check(got)  # (a) the contract, in big integers
        print(pc.format_worst(cs.prim, worst), "(%d cases, %d constructed extremes) [gfx950]" % (len(cs), cs.n_extreme))
        host = pc.run_host(primtest_host, cs)  # (b) the same code compiled for the host
        if not np.array_equal(got, host):
            i = int(np.nonzero((got != host).any(axis=1))[0][0])
            pytest.fail("%s: device and host builds of the same source disagree at case %d (%d of %d cases): device %s, host %s — a compiler "
                        "or inline-asm divergence of the device path" % (cs.prim, i, int((got != host).any(axis=1).sum()), len(cs),
                                                                         got[i].tolist(), host[i].tolist()))


def test_store_output_on_device(primtest_dev, table):
    """store_output<false> = BlsScalar limbs of V mod p; store_output<true> = raw limbs of (V 2^-256 mod p) & (2^250 - 1), for
    every tight residue -2p < V < 2p"""
    tab, lay = table
    for cs in pc.cases_for("store_output", tab, lay):
        cs.check(run_device(primtest_dev, cs))
        print("store_output<false|true>: %d cases, %d constructed extremes [gfx950]" % (len(cs), cs.n_extreme))
