"""include/chiara.h: the op / type registry "is thread-safe and needs no device".  Pinned here on the host: eight
threads fill, read and empty both tables at once.  ctypes drops the GIL inside every call, so the library really is
entered concurrently.

A refusal (CHR_ERR_UNSUPPORTED, every code taken) is only right once all 64 codes are out.  Nothing is freed while a
table is being filled, so a thread that was refused rightly has, by the time the refusal returns, been preceded by
64 creations: every successful creation of the round must have STARTED before any refusal RETURNED (host clock, taken
before a creating call and after a refused one)."""
import ctypes
import threading
import time

import chiara_amd as ca

L = ca.lib()
NTHREADS = 8
CODES = list(range(64, 128))
FN = ctypes.cast(L.chr_abi_version, ctypes.c_void_p).value  # any non-NULL function address: never called


def _op_create(_i):
    op = ctypes.c_int(-1)
    return L.chr_op_create(FN, None, 0, ctypes.byref(op)), op.value


def _type_create(count):
    t = ctypes.c_int(-1)
    return L.chr_type_contiguous(count, ca.FLOAT32, ctypes.byref(t)), t.value


def _type_size(t):
    n = ctypes.c_size_t(0)
    return L.chr_type_size(t, ctypes.byref(n)), n.value


def _run_threads(body):
    """body(thread index, barrier) in NTHREADS threads; re-raises the first exception of any of them."""
    barrier = threading.Barrier(NTHREADS)
    errors = []

    def wrap(i):
        try:
            body(i, barrier)
        except BaseException as e:  # noqa: BLE001 -- handed to the main thread
            errors.append(e)
            barrier.abort()

    threads = [threading.Thread(target=wrap, args=(i,)) for i in range(NTHREADS)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
        assert not t.is_alive(), "a registry thread did not finish"
    if errors:
        raise errors[0]


def _fill_round(create, check_mine=None):
    """Every thread creates until it is refused.  Returns per thread its codes; asserts the union and the timing."""
    mine = [[] for _ in range(NTHREADS)]
    started = [[] for _ in range(NTHREADS)]  # host clock before each successful creation
    refused_at = [None] * NTHREADS           # host clock after the refusal returned

    def body(i, barrier):
        barrier.wait()
        k = 0
        while True:
            arg = 1 + i + NTHREADS * k  # a type's count: distinct per (thread, creation), at most 8 + 8 * 64
            t0 = time.perf_counter_ns()
            rc, code = create(arg)
            if rc != 0:
                refused_at[i] = time.perf_counter_ns()
                assert rc == ca.ERR_UNSUPPORTED, rc
                break
            started[i].append(t0)
            mine[i].append((code, arg))
            if check_mine is not None:  # read back every code this thread holds while the others churn
                for c, a in mine[i]:
                    check_mine(c, a)
            k += 1
            assert k <= 64

    _run_threads(body)
    codes = [c for m in mine for c, _ in m]
    assert sorted(codes) == CODES, f"{len(codes)} codes, {len(set(codes))} distinct"
    first_refusal = min(refused_at)
    late = [t for s in started for t in s if t >= first_refusal]
    assert not late, f"{len(late)} creations began after a thread had been refused: it was refused before the table was full"
    return mine


def _free_round(mine, free):
    def body(i, barrier):
        barrier.wait()
        for code, _ in mine[i]:
            assert free(code) == 0

    _run_threads(body)


def test_op_registry_filled_and_emptied_by_eight_threads():
    for _ in range(2):  # the second round fills the table the first one emptied
        mine = _fill_round(_op_create)
        try:
            assert _op_create(0)[0] == ca.ERR_UNSUPPORTED
        finally:
            _free_round(mine, L.chr_op_free)
    for code in CODES:
        assert L.chr_op_free(code) == ca.ERR_INVALID_ARG  # every code is dead again


def test_type_registry_filled_read_and_emptied_by_eight_threads():
    def check(code, count):
        assert _type_size(code) == (0, 4 * count), (code, count, _type_size(code))

    for _ in range(2):
        mine = _fill_round(_type_create, check)
        try:
            assert _type_create(3)[0] == ca.ERR_UNSUPPORTED
            for m in mine:
                for code, count in m:
                    check(code, count)
        finally:
            _free_round(mine, L.chr_type_free)
    for code in CODES:
        assert L.chr_type_free(code) == ca.ERR_INVALID_ARG
        assert _type_size(code)[0] == ca.ERR_INVALID_ARG


def test_both_registries_churn_together():
    """Ops and types share one lock: four threads churn ops while four churn types, 200 create / read / free each; no
    call ever fails (at most 8 codes of either kind are live) and every size read back is its own."""
    def body(i, barrier):
        barrier.wait()
        for k in range(200):
            if i % 2:
                rc, op = _op_create(0)
                assert rc == 0 and 64 <= op <= 127
                assert L.chr_op_free(op) == 0
            else:
                count = 1 + i + NTHREADS * (k % 50)
                rc, t = _type_create(count)
                assert rc == 0 and 64 <= t <= 127
                assert _type_size(t) == (0, 4 * count)
                assert L.chr_type_free(t) == 0

    _run_threads(body)
