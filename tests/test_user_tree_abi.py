"""chr_op_create_tree on the host (no GPU): a user op with an optional one-pass tree launcher shares
chr_op_create's registry -- the same 64 codes, the same chr_op_free -- and the Python mirror keeps both launcher
objects alive for as long as the library holds their addresses."""
import ctypes
import gc
import re
import subprocess
import weakref

import chiara_amd as ca
from chiara_amd import _lib, collectives

FOLD_T = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                          ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)
TREE_T = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                          ctypes.c_void_p)


def _any_fn():
    return ctypes.cast(ca.lib().chr_abi_version, ctypes.c_void_p).value  # any address: never called here


def test_symbol_exported_and_listed():
    assert "chr_op_create_tree" in _lib.EXPORTED
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r"\bT chr_op_create_tree\b", out)
    assert ca.lib().chr_abi_version() == 11  # additive: the ABI number stays


def test_argument_checks():
    L = ca.lib()
    fn, op = _any_fn(), ctypes.c_int(-1)
    assert L.chr_op_create_tree(None, fn, None, 0, ctypes.byref(op)) == ca.ERR_INVALID_ARG  # the folds need fn
    assert L.chr_op_create_tree(None, None, None, 0, ctypes.byref(op)) == ca.ERR_INVALID_ARG
    assert L.chr_op_create_tree(fn, fn, None, 0, None) == ca.ERR_INVALID_ARG
    assert op.value == -1
    assert L.chr_op_create_tree(fn, None, None, 0, ctypes.byref(op)) == 0  # no tree launcher: chr_op_create
    assert 64 <= op.value <= 127
    assert L.chr_op_free(op.value) == 0


def test_both_creators_share_the_64_slots():
    L = ca.lib()
    fn, op = _any_fn(), ctypes.c_int(-1)
    made = []
    try:
        for i in range(64):
            if i % 2:
                assert L.chr_op_create(fn, None, 0, ctypes.byref(op)) == 0
            else:
                assert L.chr_op_create_tree(fn, fn, None, 0, ctypes.byref(op)) == 0
            made.append(op.value)
        assert sorted(made) == list(range(64, 128))
        assert L.chr_op_create(fn, None, 0, ctypes.byref(op)) == ca.ERR_UNSUPPORTED
        assert L.chr_op_create_tree(fn, fn, None, 0, ctypes.byref(op)) == ca.ERR_UNSUPPORTED
        # chr_op_free frees either kind; the code is handed out again, to either creator
        tree_op = made[0]
        assert L.chr_op_free(tree_op) == 0 and L.chr_op_free(tree_op) == ca.ERR_INVALID_ARG
        assert L.chr_op_create(fn, None, 1, ctypes.byref(op)) == 0 and op.value == tree_op
    finally:
        for o in made:
            L.chr_op_free(o)
    assert L.chr_op_free(made[1]) == ca.ERR_INVALID_ARG


def test_op_create_keeps_its_launchers_until_op_free():
    """A CFUNCTYPE wrapper is the only owner of its thunk: op_create must hold both objects while the library holds
    their addresses, and let go at op_free."""
    fold = FOLD_T(lambda *a: 1)
    tree = TREE_T(lambda *a: 1)
    refs = weakref.ref(fold), weakref.ref(tree)
    op = ca.op_create(fold, tree=tree)
    assert 64 <= op <= 127
    del fold, tree
    gc.collect()
    assert refs[0]() is not None and refs[1]() is not None
    assert collectives._OP_LAUNCHERS[op] == (refs[0](), refs[1]())
    assert ca.op_free(op) == 0
    gc.collect()
    assert refs[0]() is None and refs[1]() is None
    assert ca.op_free(op) == ca.ERR_INVALID_ARG
    # an address is accepted as well, and a fold-only op keeps its launcher too
    fold = FOLD_T(lambda *a: 1)
    ref = weakref.ref(fold)
    op = ca.op_create(fold)
    op2 = ca.op_create(_any_fn(), tree=_any_fn())
    del fold
    gc.collect()
    assert ref() is not None and op2 != op
    assert ca.op_free(op) == 0 and ca.op_free(op2) == 0
    gc.collect()
    assert ref() is None
