"""Circuit descriptions for the raw ABI of vp_circuit_upload (include/vpgpu.h: vp_layer_desc), the upload's contract as a Python function, and the table of
malformed descriptions that tests/test_upload_desc_host.py (CPU) and tests/test_gpu_circuit_upload.py (GPU) share.

A description is a list of per-layer dicts of numpy arrays:
    size, bit_length, ty (uint8), l (int32), u, v, lv (uint32), c ((n, 2) uint64 or None), is_assert (uint8 or None),
    dad_size (uint64[i]), dad_bitlen (int32[i]), dad_id (list of i uint32 arrays)            for layer i; layer 0 carries size and bit_length alone.
Any of the arrays may be set to None by a mutation (a NULL pointer in the C struct).  build() makes one from the seven arrays of tests/custom_circuits.py by the
reference's subset rule (layeredCircuit::subsetInit), validate() says what vp_circuit_upload must answer, to_ctypes() lays it out for the call."""
import collections
import copy
import ctypes

import numpy as np

import custom_circuits as cc

VP_OK, VP_EINVAL, VP_ELIMIT = 0, -1, -5
VP_MAX_TAB = 64
VP_BLOCK = 256
MAX_LAYER = 1 << 30
INT_MIN = -(1 << 31)
U32_MAX = (1 << 32) - 1
UNARY = (cc.MULC, cc.ADDC, cc.NOT, cc.COPY)
GATE_ARRAYS = ("ty", "l", "u", "v", "lv", "dad_size", "dad_bitlen", "dad_id")      # the arrays a gate layer must carry


class LayerDesc(ctypes.Structure):      # vp_layer_desc
    _fields_ = [("size", ctypes.c_uint64), ("bit_length", ctypes.c_int32),
                ("ty", ctypes.c_void_p), ("l", ctypes.c_void_p), ("u", ctypes.c_void_p), ("v", ctypes.c_void_p), ("lv", ctypes.c_void_p),
                ("c", ctypes.c_void_p), ("is_assert", ctypes.c_void_p),
                ("dad_size", ctypes.c_void_p), ("dad_bitlen", ctypes.c_void_p), ("dad_id", ctypes.c_void_p)]


def ceil_log2(x):
    b = 0
    while (1 << b) < x:
        b += 1
    return b


def build(layer_sizes, ty, l, u, v, c, is_assert):
    """The description of a circuit given as the seven arrays of custom_circuits.  Subsets: for layer i walk its gates from the last to the first; a binary gate's
    (l, v) met for the first time in this walk is appended to dadId[l] and lv is its position there; unary gates get l = -1 and are skipped.  c / is_assert are
    None when no gate of the layer uses them (host/prover.cpp passes NULL then)."""
    sizes = [int(s) for s in layer_sizes]
    desc, at = [], 0
    for i, n in enumerate(sizes):
        sl = slice(at, at + n)
        at += n
        if i == 0:
            desc.append({"size": n, "bit_length": ceil_log2(n)})
            continue
        t = np.asarray(ty[sl]).astype(np.uint8)
        unary = np.isin(t, UNARY)
        ll = np.where(unary, -1, np.asarray(l[sl])).astype(np.int32)
        uu = np.asarray(u[sl]).astype(np.uint32)
        vv = np.where(unary, 0, np.asarray(v[sl])).astype(np.uint32)
        lv = np.zeros(n, np.uint32)
        seen = [dict() for _ in range(i)]
        for g in range(n - 1, -1, -1):
            if unary[g]:
                continue
            pos = seen[ll[g]].setdefault(int(vv[g]), len(seen[ll[g]]))
            lv[g] = pos
        dad_id = [np.array(list(s.keys()), np.uint32) for s in seen]       # dicts keep insertion order: position = order of first use
        dad_size = np.array([len(s) for s in seen], np.uint64)
        dad_bitlen = np.array([ceil_log2(len(s)) for s in seen], np.int32)
        cc_ = np.ascontiguousarray(np.asarray(c[sl]), np.uint64).reshape(n, 2)
        aa = np.asarray(is_assert[sl]).astype(np.uint8)
        desc.append({"size": n, "bit_length": ceil_log2(n), "ty": t, "l": ll, "u": uu, "v": vv, "lv": lv,
                     "c": cc_ if np.isin(t, (cc.MULC, cc.ADDC)).any() else None, "is_assert": aa if aa.any() else None,
                     "dad_size": dad_size, "dad_bitlen": dad_bitlen, "dad_id": dad_id})
    return desc


def inputs_of(layer_sizes, u):
    """The witness of such a circuit: the input layer's u column as (n, 2) field elements (re, 0)."""
    n = int(layer_sizes[0])
    w = np.zeros((n, 2), np.uint64)
    w[:, 0] = np.asarray(u[:n], np.uint64) % np.uint64(cc.P)
    return w


def to_ctypes(desc):
    """(ctypes array of vp_layer_desc, keep-alive list).  The caller holds on to both for the duration of the call."""
    keep = []

    def ptr(a, dtype):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype)
        if a.size == 0:
            a = np.zeros(1, dtype)            # a pointer to pass; dad_size / size say that nothing is behind it
        keep.append(a)
        return a.ctypes.data
    arr = (LayerDesc * max(len(desc), 1))()
    for i, d in enumerate(desc):
        x = arr[i]
        x.size, x.bit_length = d["size"], d["bit_length"]
        if i == 0:
            continue
        for k, dt in (("ty", np.uint8), ("l", np.int32), ("u", np.uint32), ("v", np.uint32), ("lv", np.uint32), ("c", np.uint64), ("is_assert", np.uint8),
                      ("dad_size", np.uint64), ("dad_bitlen", np.int32)):
            setattr(x, k, ptr(d.get(k), dt))
        if d.get("dad_id") is not None:
            ids = (ctypes.c_void_p * max(i, 1))(*[ptr(a, np.uint32) for a in d["dad_id"]])
            keep.append(ids)
            x.dad_id = ctypes.cast(ids, ctypes.c_void_p).value
    keep.append(arr)
    return arr, keep


def validate(desc, n_layers=None):
    """The contract of vp_circuit_upload(ctx, n_layers, desc) as a function of the description: (VP_OK, None) or (code, vp_last_error text).  Text None: the
    call is refused before the library has a message for it (null arguments, fewer than two layers).  The order is the library's: the argument checks; every
    layer's size, in layer order; then layer by layer the arrays, the subsets (sizes and bit lengths by j, then the entries' range), the gates — the LOWEST failing
    gate, and within it type, u, a unary gate's l, v / l, lv — and last the constants."""
    if desc is None:
        return VP_EINVAL, None
    n = len(desc) if n_layers is None else n_layers
    if n < 2:
        return VP_EINVAL, None
    if n > VP_MAX_TAB:
        return VP_ELIMIT, "too many layers"
    for d in desc[:n]:
        if d["size"] == 0 or d["size"] > MAX_LAYER:
            return VP_ELIMIT, "bad layer size"
        if d["bit_length"] != ceil_log2(d["size"]):
            return VP_EINVAL, "bad layer size"
    size = [d["size"] for d in desc[:n]]
    for i in range(1, n):
        d = desc[i]
        if any(d.get(k) is None for k in GATE_ARRAYS):
            return VP_EINVAL, "layer arrays missing"
        ds = [int(x) for x in d["dad_size"]]
        for j in range(i):
            if ds[j] > size[j]:
                return VP_EINVAL, "dadSize too large"
            if ds[j]:
                if d["dad_id"][j] is None:
                    return VP_EINVAL, "layer arrays missing"
                if int(d["dad_bitlen"][j]) != ceil_log2(ds[j]):
                    return VP_EINVAL, "dadBitLength mismatch"
        for j in range(i):
            if ds[j] and (np.asarray(d["dad_id"][j][:ds[j]], np.int64) >= size[j]).any():
                return VP_EINVAL, "dadId out of range"
        need_c = False
        for g in range(size[i]):
            t, l, u, v, lv = int(d["ty"][g]), int(d["l"][g]), int(d["u"][g]), int(d["v"][g]), int(d["lv"][g])
            if t > cc.COPY or t == cc.INPUT:
                return VP_EINVAL, "bad gate type"
            if u >= size[i - 1]:
                return VP_EINVAL, "gate.u out of range"
            if t in UNARY:
                if l != -1:
                    return VP_EINVAL, "unary gate with l != -1"
            else:
                if l < 0 or l >= i or v >= size[l]:
                    return VP_EINVAL, "gate.v out of range"
                if lv >= ds[l] or int(d["dad_id"][l][lv]) != v:
                    return VP_EINVAL, "gate.lv inconsistent with dadId"
            need_c = need_c or t in (cc.MULC, cc.ADDC)
        if need_c and d.get("c") is None:
            return VP_EINVAL, "Addc/Mulc gates without constants"
    return VP_OK, None


# ---- the circuits the table is built on --------------------------------------------------------------------------------------------------------------
BASE_SEED, BASE_SIZES = 9, [37, 300, 257, 64, 5]


def base_arrays():
    """custom_circuits.make(BASE_SEED, BASE_SIZES): odd sizes (a padded region between size and 2^bit_length in every layer), every gate type, an assert gate per
    layer and — asserted by the host test — an empty subset in the last layer."""
    return cc.make(BASE_SEED, BASE_SIZES)


def wide_arrays():
    """A layer of 300 Add gates over 300 distinct wires: one subset of 300 entries (more than one workgroup of the range check), below a small top layer."""
    return cc.make_bucketed(5, 300, [{(cc.ADD, 0): 300}, {(cc.MUL, 1): 4, (cc.ADD, 0): 2, (cc.COPY, -1): 1}])


def no_const_arrays():
    """Neither Addc nor Mulc nor an assert gate anywhere: c and is_assert are NULL in every layer."""
    return cc.make_bucketed(6, 40, [{(cc.ADD, 0): 20, (cc.MUL, 0): 13, (cc.NOT, -1): 4, (cc.COPY, -1): 3}, {(cc.XOR, 1): 9, (cc.SUB, 0): 5, (cc.COPY, -1): 3}])


BASES = {"base": base_arrays, "wide": wide_arrays, "no_const": no_const_arrays}

Case = collections.namedtuple("Case", "name group base mutate want n_layers null_desc")
CASES = []


def _case(name, group, want, base="base", n_layers=None, null_desc=False):
    def deco(f):
        def mutate(desc):
            d = copy.deepcopy(desc)
            out = f(d)
            return d if out is None else out
        CASES.append(Case(name, group, base, mutate, want, n_layers, null_desc))
        return f
    return deco


def _gates(d, i, pred):
    L = d[i]
    return [g for g in range(L["size"]) if pred(int(L["ty"][g]), g)]


def _binary(d, i, lo=0):
    return _gates(d, i, lambda t, g: t in cc.BINARY and g >= lo)


def _last(d):
    return len(d) - 1


EINV = VP_EINVAL
# arguments
_case("desc_null", "arguments", (EINV, None), null_desc=True)(lambda d: d)
_case("one_layer", "arguments", (EINV, None), n_layers=1)(lambda d: d)
_case("layers_65", "arguments", (VP_ELIMIT, "too many layers"), n_layers=65)(lambda d: d + [copy.deepcopy(d[-1]) for _ in range(65 - len(d))])
for _where in (1, -1):
    for _k in GATE_ARRAYS:
        def _f(d, k=_k, w=_where):
            d[w if w > 0 else _last(d)][k] = None
        _case("null_%s_layer_%s" % (_k, "1" if _where > 0 else "last"), "arguments", (EINV, "layer arrays missing"))(_f)


# layer size
@_case("size_0", "layer size", (VP_ELIMIT, "bad layer size"))
def _(d):
    d[2]["size"] = 0


@_case("size_2p30_plus_1", "layer size", (VP_ELIMIT, "bad layer size"))
def _(d):
    d[_last(d)]["size"] = MAX_LAYER + 1; d[_last(d)]["bit_length"] = 31


for _name, _bl in (("bit_length_m1", lambda b: -1), ("bit_length_31", lambda b: 31), ("bit_length_below", lambda b: b - 1), ("bit_length_above", lambda b: b + 1)):
    def _f(d, f=_bl):
        d[1]["bit_length"] = f(d[1]["bit_length"])
    _case(_name, "layer size", (EINV, "bad layer size"))(_f)


@_case("bit_length_above_layer_0", "layer size", (EINV, "bad layer size"))
def _(d):
    d[0]["bit_length"] += 1


# type
for _t in (cc.INPUT, 12, 255):
    def _f(d, t=_t):
        d[2]["ty"][5] = t
    _case("type_%d" % _t, "type", (EINV, "bad gate type"))(_f)


# u
def _set_u(i, g, val):
    def f(d):
        d[i]["u"][g if g >= 0 else d[i]["size"] + g] = val(d) if callable(val) else val
    return f


_case("u_eq_size", "u", (EINV, "gate.u out of range"))(_set_u(2, 7, lambda d: d[1]["size"]))
_case("u_in_padding", "u", (EINV, "gate.u out of range"))(_set_u(2, 7, lambda d: (1 << d[1]["bit_length"]) - 1))
_case("u_u32_max", "u", (EINV, "gate.u out of range"))(_set_u(2, 7, U32_MAX))
_case("u_size_minus_1_ok", "u", (VP_OK, None))(_set_u(2, 7, lambda d: d[1]["size"] - 1))

# unary l
for _t, _tn in ((cc.ADDC, "addc"), (cc.MULC, "mulc"), (cc.NOT, "not"), (cc.COPY, "copy")):
    for _ln, _lf in (("0", lambda i: 0), ("i_minus_1", lambda i: i - 1)):
        def _f(d, t=_t, lf=_lf):
            g = _gates(d, 3, lambda ty, g: ty == t)[0]
            d[3]["l"][g] = lf(3)
        _case("unary_%s_l_%s" % (_tn, _ln), "unary l", (EINV, "unary gate with l != -1"))(_f)

# v / l
for _ln, _lf in (("m1", lambda i: -1), ("m2", lambda i: -2), ("i", lambda i: i), ("i_plus_1", lambda i: i + 1)):
    def _f(d, lf=_lf):
        d[3]["l"][_binary(d, 3)[0]] = lf(3)
    _case("binary_l_%s" % _ln, "v / l", (EINV, "gate.v out of range"))(_f)


@_case("v_eq_size", "v / l", (EINV, "gate.v out of range"))
def _(d):
    g = _binary(d, 3)[0]
    d[3]["v"][g] = d[int(d[3]["l"][g])]["size"]


@_case("v_in_padding", "v / l", (EINV, "gate.v out of range"))
def _(d):
    g = _binary(d, 3)[0]
    d[3]["v"][g] = (1 << d[int(d[3]["l"][g])]["bit_length"]) - 1


# lv
@_case("lv_eq_dad_size", "lv", (EINV, "gate.lv inconsistent with dadId"))
def _(d):
    g = _binary(d, 3)[0]
    d[3]["lv"][g] = int(d[3]["dad_size"][int(d[3]["l"][g])])


@_case("lv_u32_max", "lv", (EINV, "gate.lv inconsistent with dadId"))
def _(d):
    d[3]["lv"][_binary(d, 3)[0]] = U32_MAX


@_case("lv_swapped", "lv", (EINV, "gate.lv inconsistent with dadId"))
def _(d):
    L = d[2]
    b = _binary(d, 2)
    g = b[0]
    h = [x for x in b if L["l"][x] == L["l"][g] and L["v"][x] != L["v"][g]][0]       # the same subset, another wire: both lv stay in range
    L["lv"][g], L["lv"][h] = L["lv"][h], L["lv"][g]


def empty_subset(d):
    """(layer, j) of an empty subset of the description, the highest layer first."""
    for i in range(_last(d), 0, -1):
        for j in range(i):
            if int(d[i]["dad_size"][j]) == 0:
                return i, j
    raise AssertionError("no empty subset in this circuit")


@_case("lv_into_empty_subset", "lv", (EINV, "gate.lv inconsistent with dadId"))
def _(d):
    i, j = empty_subset(d)
    g = _binary(d, i)[0]
    d[i]["l"][g] = j; d[i]["v"][g] = 0; d[i]["lv"][g] = 0


# dadId
def _bad_dad(i, j, pos):
    def f(d):
        ids = d[i]["dad_id"][j]
        ids[pos if pos >= 0 else len(ids) + pos] = d[j]["size"]
    return f


_case("dad_id_eq_size", "dadId", (EINV, "dadId out of range"))(_bad_dad(3, 1, 2))
for _pn, _p in (("first", 0), ("last", -1), ("255", 255), ("256", 256)):
    _case("dad_id_bad_%s" % _pn, "dadId", (EINV, "dadId out of range"), base="wide")(_bad_dad(1, 0, _p))


# subsets
@_case("dad_size_above_layer", "subsets", (EINV, "dadSize too large"))
def _(d):
    n = d[1]["size"]
    d[3]["dad_size"][1] = n + 1
    d[3]["dad_id"][1] = np.arange(n + 1, dtype=np.uint32) % np.uint32(n)
    d[3]["dad_bitlen"][1] = ceil_log2(n + 1)


for _name, _dv in (("dad_bitlen_above", 1), ("dad_bitlen_below", -1)):
    def _f(d, dv=_dv):
        d[3]["dad_bitlen"][1] += dv
    _case(_name, "subsets", (EINV, "dadBitLength mismatch"))(_f)


@_case("empty_subset_bitlen_int_min_ok", "subsets", (VP_OK, None))
def _(d):
    i, j = empty_subset(d)
    d[i]["dad_bitlen"][j] = INT_MIN           # the reference stores (int) log2(0) there


# constants
for _t, _tn in ((cc.ADDC, "addc"), (cc.MULC, "mulc")):
    def _f(d, t=_t):
        L = d[3]
        keep = _gates(d, 3, lambda ty, g: ty == t)[0]
        for g in _gates(d, 3, lambda ty, g: ty in (cc.ADDC, cc.MULC)):
            if g != keep:
                L["ty"][g] = cc.COPY          # unary like the gate it replaces: l and the subsets stay as they are
        L["c"] = None
    _case("c_null_one_%s" % _tn, "constants", (EINV, "Addc/Mulc gates without constants"))(_f)
_case("c_and_assert_null_unused_ok", "constants", (VP_OK, None), base="no_const")(lambda d: d)


# placement: the same bad gate wherever a workgroup of the check begins and ends
for _i, _gs in ((1, (0, VP_BLOCK - 1, VP_BLOCK, -1)), (-1, (0, -1))):
    for _g in _gs:
        def _f(d, i=_i, g=_g):
            i = i if i > 0 else _last(d)
            d[i]["u"][g if g >= 0 else d[i]["size"] + g] = d[i - 1]["size"]
        _case("bad_u_layer_%s_gate_%s" % ("1" if _i > 0 else "last", _g if _g >= 0 else "last"), "placement", (EINV, "gate.u out of range"))(_f)


# precedence
@_case("lower_gate_wins_u_before_v", "precedence", (EINV, "gate.u out of range"))
def _(d):
    hi = _binary(d, 2, lo=1)[0]
    d[2]["v"][hi] = U32_MAX
    d[2]["u"][hi - 1] = d[1]["size"]


@_case("lower_gate_wins_v_before_u", "precedence", (EINV, "gate.v out of range"))
def _(d):
    lo = _binary(d, 2)[0]
    d[2]["v"][lo] = U32_MAX
    d[2]["u"][lo + 1] = d[1]["size"]


@_case("one_gate_u_before_v", "precedence", (EINV, "gate.u out of range"))
def _(d):
    g = _binary(d, 2)[0]
    d[2]["u"][g] = d[1]["size"]; d[2]["v"][g] = U32_MAX


@_case("lower_layer_wins", "precedence", (EINV, "bad gate type"))
def _(d):
    d[1]["ty"][3] = 12
    d[3]["u"][0] = U32_MAX


@_case("dad_id_before_the_gate_it_breaks", "precedence", (EINV, "dadId out of range"))
def _(d):
    L = d[3]
    g = _binary(d, 3)[0]                      # the entry its lv points at: the gate fails the lv check as well, at a lower index than the entry's position or not
    L["dad_id"][int(L["l"][g])][int(L["lv"][g])] = d[int(L["l"][g])]["size"]


GROUPS = tuple(dict.fromkeys(c.group for c in CASES))


def differences(a, b):
    """Where two descriptions differ: a sorted list of (layer, field) — field "dad_id[j]" per subset."""
    out = []
    for i in range(max(len(a), len(b))):
        if i >= len(a) or i >= len(b):
            out.append((i, "layer"))
            continue
        for k in ("size", "bit_length", "ty", "l", "u", "v", "lv", "c", "is_assert", "dad_size", "dad_bitlen"):
            x, y = a[i].get(k), b[i].get(k)
            if (x is None) != (y is None) or (x is not None and not np.array_equal(np.asarray(x), np.asarray(y))):
                out.append((i, k))
        x, y = a[i].get("dad_id"), b[i].get("dad_id")
        if (x is None) != (y is None):
            out.append((i, "dad_id"))
        elif x is not None:
            for j in range(max(len(x), len(y))):
                if j >= len(x) or j >= len(y) or not np.array_equal(x[j], y[j]):
                    out.append((i, "dad_id[%d]" % j))
    return sorted(out)
