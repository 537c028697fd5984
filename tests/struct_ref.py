"""Expected values of the derived-type tests (tests/test_gpu_struct_op.py) in numpy: the functors of
tests/userop/struct_op.hip on elements of K consecutive base values, folds, the post-order tree program and the plan
interpreter, each with the arithmetic passed in.  Buffers are flat arrays of the base type; an element is a row of the
(n, K) view.  tests/test_type_contiguous_host.py checks the HalfAdd paths against the oracle's user_halfadd."""
import numpy as np

import chiara_amd as ca


def _mix1(x, y):
    """halfadd_op.hip's arithmetic: x * 0.5 + y rounded after the multiply; 3 * x + y wrapping at the base width."""
    if x.dtype.kind == "f":
        h = x * x.dtype.type(0.5)
        return h + y
    u = np.dtype(f"u{x.dtype.itemsize}")
    with np.errstate(over="ignore"):
        return (x.view(u) * u.type(3) + y.view(u)).view(x.dtype)


def halfadd(x, y):
    """HalfAddK: in o inout per component.  x, y: (n, K)."""
    return _mix1(np.ascontiguousarray(x), np.ascontiguousarray(y))


def rotmix(x, y):
    """RotMixK: r.v[i] = in.v[(i + 1) % K] o inout.v[i]."""
    return _mix1(np.ascontiguousarray(np.roll(x, -1, axis=1)), np.ascontiguousarray(y))


def _rows(a, k):
    return np.ascontiguousarray(a).reshape(-1, k)


def fold_ref(acc, ins, k, f, running_first):
    """chr_user_reduce_fn: ins[m-1] o (... (ins[0] o acc)), or running value first (((acc o ins[0]) o ins[1]) ...)."""
    r = _rows(acc, k).copy()
    for x in ins:
        r = f(r, _rows(x, k)) if running_first else f(_rows(x, k), r)
    return r.reshape(-1)


def tree_ref(leaves, comb, swaps, k, f):
    """chr_reduce_tree's program: push leaf j, then comb[j] combines; a combine pops `top` and folds it into the
    running value below: run = top o run, or with its swap bit run = run o top."""
    stack, ci = [], 0
    for j, leaf in enumerate(leaves):
        stack.append(_rows(leaf, k).copy())
        for _ in range(comb[j]):
            top = stack.pop()
            run = stack.pop()
            stack.append(f(run, top) if swaps[ci] else f(top, run))
            ci += 1
    assert len(stack) == 1
    return stack[0].reshape(-1)


# ---- the plan interpreter: tests/plan_sim.py's loop over (count, K) buffers with the arithmetic passed in ---------

def _view(bufs, ref, n):
    name, off = ref
    return bufs[name][off:off + n]


def _run_local(bufs, op, k, f):
    kind, dst, acc, n, ins = op[:5]
    if n == 0:
        return
    if kind == "tree":
        comb, swaps = op[5]
        leaves = [_view(bufs, ref, n) for ref in [acc] + list(ins)]
        _view(bufs, dst, n)[:] = tree_ref(leaves, comb, swaps, k, f).reshape(-1, k)
    elif kind == "copy2d":
        rows, dp, sp = ins
        for r in range(rows):
            _view(bufs, (dst[0], dst[1] + r * dp), n)[:] = _view(bufs, (acc[0], acc[1] + r * sp), n).copy()
    elif kind == "copy":
        _view(bufs, dst, n)[:] = _view(bufs, acc, n).copy()
    else:
        _view(bufs, dst, n)[:] = fold_ref(_view(bufs, acc, n), [_view(bufs, r, n).copy() for r in ins], k, f,
                                          kind == "reduce_sw").reshape(-1, k)


def execute(plans, sends, k, f, inplace=False):
    """Every rank's RECV buffer after the plans ran; sends[r]: flat base-type array of whole elements."""
    n = len(plans)
    states = []
    for r in range(n):
        h = plans[r]["header"]
        send = _rows(sends[r], k).copy()
        recv = send if inplace else np.zeros((h["recv"], k), dtype=send.dtype)
        states.append({"SEND": send, "RECV": recv, "ACC": np.zeros((h["acc"], k), dtype=send.dtype),
                       "STAGE": np.zeros((max(h["stage"], 1), k), dtype=send.dtype)})
    for r in range(n):
        for op in plans[r]["pre"]:
            _run_local(states[r], op, k, f)
    nsteps = len(plans[0]["steps"])
    assert all(len(p["steps"]) == nsteps for p in plans)
    for si in range(nsteps):
        used = [[False] * len(plans[r]["steps"][si]["sends"]) for r in range(n)]
        payload = []
        for r in range(n):
            for peer, ref, cnt in plans[r]["steps"][si]["recvs"]:
                qs = plans[peer]["steps"][si]["sends"]
                j = next(j for j, s in enumerate(qs) if not used[peer][j] and s[0] == r)
                assert qs[j][2] == cnt, "send/recv size mismatch"
                used[peer][j] = True
                payload.append((r, ref, _view(states[peer], qs[j][1], cnt).copy()))
        assert all(all(u) for u in used), f"unmatched send in step {si}"
        for r, ref, data in payload:
            _view(states[r], ref, data.shape[0])[:] = data
        for ci in range(len(plans[0]["steps"][si].get("allgathers", []))):
            blocks = []
            for r in range(n):
                (buf, off), cnt = plans[r]["steps"][si]["allgathers"][ci]
                blocks.append(_view(states[r], (buf, off + r * cnt), cnt).copy())
            for r in range(n):
                (buf, off), cnt = plans[r]["steps"][si]["allgathers"][ci]
                for q in range(n):
                    _view(states[r], (buf, off + q * cnt), cnt)[:] = blocks[q]
        for r in range(n):
            for op in plans[r]["steps"][si]["post"]:
                _run_local(states[r], op, k, f)
    return [st["RECV"].reshape(-1) for st in states]


def simulate(mode, sends, k_radix, b, k, f, inplace=False, slices=1, schedule=None, commutative=False):
    """The collective `mode` over derived elements of k base values (count in derived elements from sends[0])."""
    n = len(sends)
    rs = mode in ca.RS_MODES
    count = sends[0].size // k // n if rs else sends[0].size // k
    plans = [ca.parse_plan(ca.describe_plan(mode, n, r, k_radix, b, count, slices, schedule, commutative))
             for r in range(n)]
    if plans[0]["header"]["error"]:
        raise ValueError(f"plan error {plans[0]['header']['error']}", plans[0]["header"]["error"])
    outs = execute(plans, sends, k, f, inplace)
    if rs:
        outs = [o[:count * k] for o in outs]
    return outs
