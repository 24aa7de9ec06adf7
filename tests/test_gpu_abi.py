"""GPU: what a context holds on the device (include/apd_hip.h apd_device_bytes, apd_device_mem_info).

* apd_device_bytes is the context's own count of its buffers: 0 before a problem, positive after a
  run, unchanged by a second set_problem + run of the same problem (every buffer is reused).
* create / job / destroy cycles of the two contexts with the most buffers (apd_ctx, apd_eval_ctx)
  give the device its memory back: over ten cycles free memory falls by less than half of one
  cycle's footprint, where a buffer set leaked per cycle would cost ten footprints. The engine's ten
  cycles cost one 32 MiB block of the runtime's own whatever the buffers do (measured with the
  hand-kept free lists this test came after, and the same since): its margin is that block plus half
  a footprint, still a sixth of what a leak would take (footprint 33 169 656 bytes at 384 x 288).
"""
import ctypes as C

import numpy as np
import pytest

import apd_abi as A
import cases

pytestmark = pytest.mark.gpu

# what one EvalEngine.set_target + distances of _eval_job() takes from the device's free memory
# (measured once as that drop, in a process whose kernels are loaded; the context has no byte accessor)
EVAL_FOOTPRINT = 123_731_968
# free memory the runtime itself keeps over ten cycles, none of it the contexts' buffers
RUNTIME_DRIFT = {"engine": 32 << 20, "eval": 0}


@pytest.fixture(scope="module")
def lib():
    lib = A.load_library()
    if lib.apd_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return lib


def free_bytes(probe):
    free, total = C.c_size_t(), C.c_size_t()
    probe._check(probe.lib.apd_device_mem_info(probe.ctx, C.byref(free), C.byref(total)), "apd_device_mem_info")
    return free.value


def test_device_bytes_counts_the_buffers_held(lib):
    arr = cases.base_problem(cases.scene(96, 72, 4), 0)
    eng = A.Engine(0, lib)
    try:
        assert eng.device_bytes() == 0
        eng.set_problem(arr)
        eng.run()
        held = eng.device_bytes()
        print(f"apd_device_bytes after the 96x72 N=4 problem: {held}")
        assert held > 0
        eng.set_problem(arr)
        eng.run()
        assert eng.device_bytes() == held
    finally:
        eng.close()


def _engine_job(lib, arr):
    eng = A.Engine(0, lib)
    try:
        eng.set_problem(arr)
        eng.run()
        return eng.device_bytes()
    finally:
        eng.close()


def _eval_job(lib, clouds):
    target, query = clouds
    ev = A.EvalEngine(0, lib)
    try:
        ev.set_target(target)
        ev.distances(query, 0.05)
        return EVAL_FOOTPRINT
    finally:
        ev.close()


@pytest.mark.parametrize("kind", ["engine", "eval"])
def test_create_destroy_cycles_return_the_memory(lib, kind):
    if kind == "engine":
        job, arg = _engine_job, cases.base_problem(cases.scene(384, 288, 4), 0)
    else:
        rng = np.random.default_rng(7)
        job, arg = _eval_job, (rng.random((200_000, 3), dtype=np.float32), rng.random((2_000_000, 3), dtype=np.float32))
    probe = A.Engine(0, lib)  # holds no buffer: only reads the device's free memory
    try:
        footprint = job(lib, arg)  # the warm-up cycle
        before = free_bytes(probe)
        for _ in range(10):
            job(lib, arg)
        drift = before - free_bytes(probe)
        print(f"{kind}: footprint {footprint} bytes, free memory fell by {drift} bytes over 10 cycles")
        assert footprint > 0
        assert drift < RUNTIME_DRIFT[kind] + footprint // 2
    finally:
        probe.close()
