"""dymu_batch_reduce_device and dymu_level_mask_device on constructed stacks.

No solve runs here: synthetic planes are uploaded in the batch layout (plane pitch P rows,
wall rows below every plane) and the kernels' outputs are compared bit for bit with the
numpy fold the header defines, in the same order.  The wall rows hold -1.0 and the padding
columns a negative sentinel, so a kernel that read either would win every MIN and the
summary; the padding of the outputs holds sentinels that must survive.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INF = np.inf
NONE = 0xFFFFFFFF
SUM, MAX, MIN = 0, 1, 2
NX, NY = 97, 61
PAD_IN, PAD_OUT, PAD_ARG, PAD_MASK = -3.0, -12345.0, 0xABABABAB, 0xCC


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the reference: the header's fold, plane by plane in the listed order ----
def fold(planes, ids, op, w=None, o=None):
    acc = arg = None
    for k, (T, p) in enumerate(zip(planes, ids)):
        t = T
        if w is not None:
            t = w[k] * t
        if o is not None:
            t = t + o[k]
        if k == 0:
            acc, arg = np.array(t, dtype=np.float64), np.full(T.shape, p, dtype=np.uint32)
        elif op == SUM:
            acc = acc + t
        else:
            m = t > acc if op == MAX else t < acc
            acc, arg = np.where(m, t, acc), np.where(m, np.uint32(p), arg)
    if op == MIN:
        arg = np.where(acc == INF, np.uint32(NONE), arg)
    return acc, arg


def summary_ref(out, arg, op):
    fin = out < INF
    if not fin.any():
        return dict(min_value=INF, min_i=NONE, min_j=NONE, min_plane=NONE, n_finite=0)
    v = out[fin].min()
    k = int(np.flatnonzero(fin.ravel() & (out.ravel() == v))[0])  # the lowest row-major cell
    j, i = divmod(k, out.shape[1])
    return dict(min_value=float(out[j, i]), min_i=i, min_j=j,
                min_plane=NONE if op == SUM else int(arg[j, i]), n_finite=int(fin.sum()))


def same_summary(got, ref):
    assert np.float64(got["min_value"]).view(np.uint64) == np.float64(ref["min_value"]).view(np.uint64)
    for k in ("min_i", "min_j", "min_plane", "n_finite"):
        assert got[k] == ref[k], (k, got, ref)


# ---- a stack on the device ----
class Stack:
    """planes (list of [ny, nx]) in the batch layout with pitch ld, at an offset of `skew`
    doubles from the allocation (skew = 1: every row of an even pitch starts 8 bytes off)."""

    def __init__(self, dymu, eng, planes, ld, skew=0):
        self.eng, self.B = eng, len(planes)
        self.ny, self.nx = planes[0].shape
        self.ld, self.P = ld, dymu.batch_plane_rows(self.ny)
        self.host = np.full((self.B * self.P, ld), PAD_IN)
        for b, T in enumerate(planes):
            self.host[b * self.P:b * self.P + self.ny, :self.nx] = T
            self.host[b * self.P + self.ny:(b + 1) * self.P, :self.nx] = -1.0  # wall rows
        self.base = eng.alloc(self.host.nbytes + 8 * skew)
        self.ptr = self.base + 8 * skew
        eng.h2d(self.ptr, self.host)

    def unchanged(self):
        back = np.empty_like(self.host)
        self.eng.d2h(back, self.ptr)
        return np.array_equal(bits(back), bits(self.host))

    def free(self):
        self.eng.free(self.base)


class Outputs:
    """Sentinel-filled d_out / d_arg with their own pitches."""

    def __init__(self, eng, nx, ny, out_ld, arg_ld=None):
        self.eng, self.nx, self.ny = eng, nx, ny
        self.out_ld, self.arg_ld = out_ld, arg_ld or nx
        self.out0 = np.full((ny, self.out_ld), PAD_OUT)
        self.arg0 = np.full((ny, self.arg_ld), PAD_ARG, dtype=np.uint32)
        self.d_out, self.d_arg = eng.alloc(self.out0.nbytes), eng.alloc(self.arg0.nbytes)
        eng.h2d(self.d_out, self.out0)
        eng.h2d(self.d_arg, self.arg0)

    def read(self):
        out, arg = np.empty_like(self.out0), np.empty_like(self.arg0)
        self.eng.d2h(out, self.d_out)
        self.eng.d2h(arg, self.d_arg)
        return out, arg

    def untouched(self):
        out, arg = self.read()
        return np.array_equal(bits(out), bits(self.out0)) and np.array_equal(arg, self.arg0)

    def free(self):
        self.eng.free(self.d_out)
        self.eng.free(self.d_arg)


def run(eng, st, op, outs, planes=None, weights=None, offsets=None, with_arg=True):
    return eng.batch_reduce(st.ptr, st.nx, st.ny, st.B, st.ld, op, planes=planes, weights=weights,
                            offsets=offsets, d_out=outs.d_out, out_ld=outs.out_ld,
                            d_arg=outs.d_arg if with_arg else 0,
                            arg_ld=outs.arg_ld if with_arg else 0)


def check(eng, st, host_planes, op, outs, planes=None, weights=None, offsets=None):
    """One call against the fold: out bit-identical, arg equal, the summary equal, every
    sentinel and the stack intact."""
    arg_before = outs.read()[1]  # an earlier call's plane map, or the sentinels
    s = run(eng, st, op, outs, planes, weights, offsets)
    ids = list(range(st.B)) if planes is None else list(planes)
    ref, ref_arg = fold([host_planes[p] for p in ids], ids, op, weights, offsets)
    out, arg = outs.read()
    nx = st.nx
    assert np.array_equal(bits(out[:, :nx]), bits(ref))
    assert np.array_equal(bits(out[:, nx:]), bits(outs.out0[:, nx:]))
    if op == SUM:
        assert np.array_equal(arg, arg_before)  # a sum writes no plane map
    else:
        assert np.array_equal(arg[:, :nx], ref_arg)
        assert np.array_equal(arg[:, nx:], outs.arg0[:, nx:])
    same_summary(s, summary_ref(ref, ref_arg, op))
    assert st.unchanged()
    return ref, ref_arg, s


def random_planes(rng, B, ny, nx, common_inf=0.01):
    """Doubles in [0, 100) spread over six decades, about 5 % +inf per plane, and cells
    that are +inf in every plane."""
    common = rng.random((ny, nx)) < common_inf
    planes = []
    for _ in range(B):
        T = rng.random((ny, nx)) * 100.0 * 10.0 ** -rng.integers(0, 6, (ny, nx)).astype(np.float64)
        T[rng.random((ny, nx)) < 0.04] = INF
        T[common] = INF
        T.setflags(write=False)
        planes.append(T)
    return planes


@pytest.fixture(scope="module")
def planes5():
    p = random_planes(np.random.default_rng(514), 5, NY, NX)
    allinf = np.logical_and.reduce([np.isinf(T) for T in p])
    assert allinf.any() and all(np.isinf(T).mean() > 0.03 for T in p)
    return p


@pytest.fixture(scope="module")
def stacks(dymu, engine, planes5):
    """The B = 5 stack at both pitches; a call with B < 5 reads its first planes."""
    st = {ld: Stack(dymu, engine, planes5, ld) for ld in (97, 104)}
    assert st[97].P == 64
    yield st
    for s in st.values():
        s.free()


class FirstPlanes:
    """The first B planes of a stack, as a stack of its own."""

    def __init__(self, st, B):
        self.__dict__.update(st.__dict__)
        self.B, self._st = B, st

    def unchanged(self):
        return self._st.unchanged()


# ---- 1. parity ----
@pytest.mark.parametrize("out_ld", [97, 100])
@pytest.mark.parametrize("ld", [97, 104])
@pytest.mark.parametrize("B", [1, 2, 3, 5])
@pytest.mark.parametrize("op", [SUM, MAX, MIN])
def test_parity(engine, stacks, planes5, op, B, ld, out_ld):
    outs = Outputs(engine, NX, NY, out_ld, arg_ld=out_ld + 1)
    try:
        check(engine, FirstPlanes(stacks[ld], B), planes5, op, outs)
    finally:
        outs.free()


def test_parity_odd_base(dymu, engine, planes5):
    """An even pitch from an address 8 bytes off a 16-byte boundary: every row has a head
    cell; and outputs whose pairs are never 16-byte aligned."""
    st = Stack(dymu, engine, planes5[:3], 104, skew=1)
    outs = Outputs(engine, NX, NY, 98, arg_ld=98)
    try:
        for op in (SUM, MAX, MIN):
            check(engine, st, planes5, op, outs)
    finally:
        outs.free()
        st.free()


def test_without_arg_map_and_without_summary(engine, stacks, planes5):
    st = stacks[97]
    outs = Outputs(engine, NX, NY, 100)
    try:
        s = run(engine, st, MIN, outs, with_arg=False)
        ref, ref_arg = fold(planes5, range(5), MIN)
        out, arg = outs.read()
        assert np.array_equal(bits(out[:, :NX]), bits(ref)) and np.array_equal(arg, outs.arg0)
        same_summary(s, summary_ref(ref, ref_arg, MIN))  # min_plane without an arg map
        r = engine.batch_reduce(st.ptr, NX, NY, 5, 97, MAX, d_out=outs.d_out, out_ld=100,
                                summary=False)
        assert r is None
        out, _ = outs.read()  # the download is ordered after the kernel
        assert np.array_equal(bits(out[:, :NX]), bits(fold(planes5, range(5), MAX)[0]))
        assert engine.last_reduce_ms() > 0.0
    finally:
        outs.free()


# ---- 2. plane lists ----
def test_plane_lists(engine, stacks, planes5):
    st = stacks[97]
    outs = Outputs(engine, NX, NY, 97)
    perm = [4, 2, 0, 3, 1]
    a, b = fold(planes5, range(5), SUM)[0], fold([planes5[p] for p in perm], perm, SUM)[0]
    assert (bits(a) != bits(b)).any()  # the order is part of a sum's bits
    w, o = [0.5, 3.0, 1.25e-3], [0.0, 7.5, 1e-9]
    try:
        for op in (SUM, MAX, MIN):
            check(engine, st, planes5, op, outs, planes=[3, 1])
            check(engine, st, planes5, op, outs, planes=perm)
            check(engine, st, planes5, op, outs, planes=[2, 0, 2, 4, 2, 2])
            check(engine, st, planes5, op, outs, planes=[4, 0, 1], weights=w)
            check(engine, st, planes5, op, outs, planes=[4, 0, 1], offsets=o)
            check(engine, st, planes5, op, outs, planes=[4, 0, 1], weights=w, offsets=o)
            check(engine, st, planes5, op, outs, weights=[1.5, 2.5, 0.1, 7.0, 3.0],
                  offsets=[0.0, 0.5, 0.25, 1e3, 2.0])
    finally:
        outs.free()


# ---- 3. ties and none ----
def test_ties_and_none(dymu, engine):
    rng = np.random.default_rng(77)
    tie = [rng.integers(0, 3, (NY, NX)).astype(np.float64) for _ in range(3)]
    const = [np.full((NY, NX), 2.0), np.full((NY, NX), 2.0)]
    none = [np.full((NY, NX), INF)]
    planes = tie + const + none
    st = Stack(dymu, engine, planes, 97)
    outs = Outputs(engine, NX, NY, 97)
    try:
        order = [2, 0, 1]
        equal = (tie[0] == tie[1]) & (tie[1] == tie[2])
        assert equal.sum() > 100
        for op in (MAX, MIN):
            _, arg, _ = check(engine, st, planes, op, outs, planes=order)
            assert (arg[equal] == 2).all()  # the first listed plane
        for op in (SUM, MAX, MIN):
            _, _, s = check(engine, st, planes, op, outs, planes=[3, 4])
            assert (s["min_i"], s["min_j"]) == (0, 0) and s["n_finite"] == NX * NY
            _, arg, s = check(engine, st, planes, op, outs, planes=[5, 5])
            assert s == dict(min_value=INF, min_i=NONE, min_j=NONE, min_plane=NONE, n_finite=0)
            if op == MIN:
                assert (arg == NONE).all()
    finally:
        outs.free()
        st.free()


# ---- 4. small and large shapes ----
@pytest.mark.parametrize("nx,ny,ld", [(1, 1, 1), (7, 1, 7), (1, 7, 1), (2, 3, 3)])
def test_small_shapes(dymu, engine, nx, ny, ld):
    planes = random_planes(np.random.default_rng(nx * 10 + ny), 2, ny, nx, common_inf=0.0)
    st = Stack(dymu, engine, planes, ld)
    outs = Outputs(engine, nx, ny, nx + 1, arg_ld=nx + 2)
    try:
        for op in (SUM, MAX, MIN):
            check(engine, st, planes, op, outs)
    finally:
        outs.free()
        st.free()


def test_large_shape_more_than_one_trip(dymu, engine):
    """1537 x 1031, B = 2: 4124 tiles for at most 2048 workgroups, so the grid-stride loop
    takes more than one trip; the summary's minimum is planted in the last row."""
    nx, ny = 1537, 1031
    rng = np.random.default_rng(9)
    planes = [1.0 + rng.random((ny, nx)) * 50.0 for _ in range(2)]
    for T in planes:
        T[rng.random((ny, nx)) < 0.02] = INF
    planes[0][ny - 1, 1201], planes[1][ny - 1, 1201] = 0.25, 0.5
    st = Stack(dymu, engine, planes, nx)
    outs = Outputs(engine, nx, ny, nx)
    try:
        for op in (SUM, MAX, MIN):
            _, _, s = check(engine, st, planes, op, outs)
            assert (s["min_i"], s["min_j"]) == (1201, ny - 1)
    finally:
        outs.free()
        st.free()


# ---- 5. level mask ----
def level_mask(engine, m, ld, mask_ld, bound):
    ny, nx = m.shape
    host = np.full((ny, ld), PAD_IN)
    host[:, :nx] = m
    mask0 = np.full((ny, mask_ld), PAD_MASK, dtype=np.uint8)
    d_map, d_mask = engine.alloc(host.nbytes), engine.alloc(mask0.nbytes)
    try:
        engine.h2d(d_map, host)
        engine.h2d(d_mask, mask0)
        r = engine.level_mask(d_map, nx, ny, ld, bound, d_mask, mask_ld)
        mask = np.empty_like(mask0)
        engine.d2h(mask, d_mask)
    finally:
        engine.free(d_map)
        engine.free(d_mask)
    assert (mask[:, nx:] == PAD_MASK).all()
    return mask[:, :nx], r


def mask_ref(m, bound):
    ref = (m <= bound).astype(np.uint8)
    jj, ii = np.nonzero(ref)
    box = (ii.min(), jj.min(), ii.max(), jj.max()) if len(ii) else None
    return ref, box, int(ref.sum())


@pytest.mark.parametrize("ld,mask_ld", [(97, 97), (104, 100), (97, 99)])
def test_level_mask(engine, planes5, ld, mask_ld):
    m = fold(planes5[:2], [0, 1], SUM)[0]
    fin = m[m < INF]
    exact = float(np.sort(fin)[len(fin) // 3])  # a bound equal to a cell's value
    for bound in (exact, float(np.median(fin)) * 1.01, float(fin.max()), 1e300):
        mask, r = level_mask(engine, m, ld, mask_ld, bound)
        ref, box, n = mask_ref(m, bound)
        assert np.array_equal(mask, ref)
        assert r["n_range"] == n and r["box"] == box and r["r_const"] == 0.0
    jj, ii = np.nonzero(m == exact)
    mask, _ = level_mask(engine, m, ld, mask_ld, exact)
    assert mask[jj[0], ii[0]] == 1
    mask, r = level_mask(engine, m, ld, mask_ld, float(fin.min()) * 0.5)
    assert r["n_range"] == 0 and r["box"][0] > r["box"][2] and not mask.any()


def test_level_mask_small_box(engine):
    """A sub-level set of a few cells: the box is theirs."""
    m = np.full((NY, NX), 9.0)
    m[17, 5], m[40, 90], m[22, 96] = 1.0, 2.0, 2.5
    mask, r = level_mask(engine, m, 97, 97, 2.5)
    assert r["box"] == (5, 17, 96, 40) and r["n_range"] == 3 and mask.sum() == 3
    with pytest.raises(Exception):
        level_mask(engine, m, 97, 97, INF)
    with pytest.raises(Exception):
        level_mask(engine, m, 97, 97, float("nan"))
    with pytest.raises(Exception):
        level_mask(engine, m, 97, 96, 1.0)  # mask_ld < nx


# ---- 6. bad arguments touch nothing ----
def test_bad_arguments_touch_nothing(dymu, engine, stacks):
    st = stacks[104]
    outs = Outputs(engine, NX, NY, 100, arg_ld=100)
    fn = engine._lib.dymu_batch_reduce_device
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)

    def rc(**kw):
        a = dict(ctx=engine.ctx, stack=st.ptr, nx=NX, ny=NY, B=5, ld=104, op=SUM, planes=None,
                 n_planes=0, weights=None, offsets=None, d_out=outs.d_out, out_ld=100,
                 d_arg=outs.d_arg, arg_ld=100)
        a.update(kw)
        keep = [a[k] for k in ("planes", "weights", "offsets")]
        ptr = [None if v is None else v.ctypes.data for v in keep]
        s = dymu.DymuReduceSummary()
        return fn(a["ctx"], a["stack"], a["nx"], a["ny"], a["B"], a["ld"], a["op"], ptr[0],
                  a["n_planes"], ptr[1], ptr[2], a["d_out"], a["out_ld"], a["d_arg"], a["arg_ld"],
                  ctypes.byref(s), None)

    try:
        assert rc() == 0  # the template call is a good one
        engine.h2d(outs.d_out, outs.out0)
        bad = [dict(ctx=None), dict(stack=None), dict(d_out=None), dict(nx=0), dict(ny=0),
               dict(B=0), dict(ld=96), dict(out_ld=96), dict(arg_ld=96), dict(op=3), dict(op=-1),
               dict(planes=u32([0]), n_planes=0), dict(planes=u32(np.zeros(65537)), n_planes=65537),
               dict(planes=u32([0, 5]), n_planes=2), dict(ny=1 << 20, B=1 << 13)]
        for w in (0.0, -1.0, INF, float("nan")):
            bad.append(dict(planes=u32([0, 1]), n_planes=2, weights=f64([1.0, w])))
        for o in (-1.0, INF, float("nan")):
            bad.append(dict(planes=u32([0, 1]), n_planes=2, offsets=f64([0.0, o])))
        # d_out inside the stack, and ending in its first bytes
        bad += [dict(d_out=st.ptr + 8 * 104 * 70), dict(d_out=st.ptr - 8 * (100 * (NY - 1) + NX) + 8),
                dict(d_arg=st.ptr + 64)]
        for kw in bad:
            assert rc(**kw) == -1, kw
        assert outs.untouched() and st.unchanged()
    finally:
        outs.free()


# ---- 7. run to run ----
def test_run_to_run(engine, stacks, planes5):
    st = stacks[97]
    outs = Outputs(engine, NX, NY, 97)
    try:
        for op in (SUM, MAX, MIN):
            s1 = run(engine, st, op, outs, weights=[1.5, 2.5, 0.1, 7.0, 3.0])
            o1, a1 = outs.read()
            s2 = run(engine, st, op, outs, weights=[1.5, 2.5, 0.1, 7.0, 3.0])
            o2, a2 = outs.read()
            assert np.array_equal(bits(o1), bits(o2)) and np.array_equal(a1, a2)
            same_summary(s1, s2)
    finally:
        outs.free()
