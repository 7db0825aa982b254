"""Support for tests/test_probe_emu.py and tests/test_probe_gpu.py: the argument sets, the references and the bindings of the probe
(csrc/mp2_probe.h: every device-path form of csrc/tl_libm.h and every cross-lane primitive of csrc/mp2_wave.h, one by one).

* libm forms: 2^20 arguments per form from numpy.random.default_rng, the distributions of tools/libm_agree.cpp worker() restated inside
  each form's stated domain (the encoder's ranges, every binade of the domain, the neighbourhoods of the routines' branch points), plus
  a short deterministic edge list.  The reference is THIS machine's libm through a C shim (tests/emu/libm_ref.c) -- never numpy's
  transcendentals, which are not glibc's.
* wave primitives: 4096 random cases of 64 lanes per primitive plus constructed ones; the oracles are plain numpy written from the
  comments of mp2_wave.h (what the primitive MEANS), not from its tlh_* loops.
* the emulation: tests/emu/mp2_probe_emu.cpp (the same mp2_probe.h with -DTL_EMULATE), compiled into a temporary directory at first use."""
import ctypes as C
import subprocess
import tempfile
from pathlib import Path

import numpy as np

from loudnesslib import GXX

ROOT = Path(__file__).resolve().parent.parent
NRANDOM = 1 << 20
NWAVES = 4096
ERR_ARG = 18
U64 = np.uint64
ALL1 = U64(0xffffffffffffffff)
SPECIAL_LANES = (0, 1, 14, 15, 16, 17, 31, 32, 33, 47, 48, 62, 63)

# form -> (code in csrc/mp2_probe.h, takes b, returns r1, table placements)
FORMS = {
    "log_pn": (0, False, False, (0, 1)), "log10_pn": (1, False, False, (0, 1)), "log10_split": (2, False, False, (0, 1)),
    "pow10_sl": (3, False, False, (0,)), "exp_sl": (4, False, False, (0,)), "sincos_sl": (5, False, True, (0,)),
    "sincos_phased": (6, False, True, (0,)), "sincos_phased_raw": (7, True, True, (0,)), "atan2_phased": (8, True, False, (0,)),
    "atan2_ns": (9, True, False, (0,)), "div_ns": (10, True, False, (0,)), "sqrt_ns": (11, False, False, (0,)),
    "sqrt_nz": (12, False, False, (0,)), "rcp_seed": (13, False, False, (0,)), "rsq_seed": (14, False, False, (0,)),
    "div": (15, True, False, (0,)), "sqrt": (16, False, False, (0,)), "min_nn": (17, True, False, (0,)),
    "max_nn": (18, True, False, (0,)), "fma_k": (19, True, False, (0,)), "recip": (20, False, False, (0,)),
}
NFORMS = 21
SEEDS = ("rcp_seed", "rsq_seed")        # the two halves differ here by design (hardware seed / exact reciprocal): their check is the error bound
# ... and so does the reciprocal refined from the seed.  Its bound: two Newton steps take a seed error e <= 2^-20 to e^4 = 2^-80; what is left is
# the rounding of the last step, r + r e' with |e'| < 2^-40 (its own rounding is below 2^-93): one rounding of r, 2^-53 relative.  2^-52 has a
# factor of two to spare; ONE step from the hardware's 2^-24 seed leaves 2^-48.
NOT_BIT_EQUAL = SEEDS + ("recip",)
SEED_BOUND = {"rcp_seed": 2.0 ** -20, "rsq_seed": 2.0 ** -20, "recip": 2.0 ** -52}
FMA_K = float(np.array([0xbfd5555555555555], dtype=U64).view(np.float64)[0])
PRIMS = {
    "wave_min_u64": 0, "wave_argmin_u64": 1, "wave_sum_i32": 2, "wave_xor_u32": 3, "wave_exscan_i32": 4, "wave_incl_xscan_u32": 5,
    "row16_max_f64": 6, "par_min_u64": 7, "par_sum_i32": 8, "ballot": 9, "rank_below": 10, "swap1_u64": 11, "swap1_f64": 12,
    "rot32_f64": 13, "mirror1": 14, "mirror4": 15, "other": 16, "readlane_i32": 17, "uni_i": 18, "select": 19, "sign_bit": 20, "ld2st2": 21,
}
NPRIMS = 22
PRIM_TWO_IN = ("other", "readlane_i32", "select", "ld2st2")

# ------------------------------------------------------------------------------------------------------------------------------------
# native pieces
_built = {}


def _build(name, args):
    if name not in _built:
        out = Path(tempfile.mkdtemp(prefix="probe")) / name
        subprocess.run(args + ["-o", str(out)], check=True)
        _built[name] = C.CDLL(str(out))
    return _built[name]


def emu():
    """tests/emu/mp2_probe_emu.cpp, the flags of the other emulations (tests/loudnesslib.py GXX)"""
    L = _build("libmp2probeemu.so", GXX + ["-shared", str(ROOT / "tests" / "emu" / "mp2_probe_emu.cpp"), "-lm"])
    bind_probe(L.probe_libm, L.probe_wave)
    return L


def ref():
    """tests/emu/libm_ref.c: this machine's libm.so.6 over arrays"""
    L = _build("libmref.so", ["gcc", "-O1", "-fno-builtin", "-ffp-contract=off", "-fPIC", "-shared", str(ROOT / "tests" / "emu" / "libm_ref.c"), "-lm"])
    for f in ("ref_log", "ref_log10", "ref_exp", "ref_pow10", "ref_sqrt"):
        getattr(L, f).argtypes = [C.c_long, C.c_void_p, C.c_void_p]
    for f in ("ref_sincos", "ref_atan2", "ref_div"):
        getattr(L, f).argtypes = [C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ref_fma.argtypes = [C.c_long, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    return L


def bind_probe(libm_fn, wave_fn):
    libm_fn.argtypes = [C.c_int, C.c_int, C.c_long] + [C.c_void_p] * 4
    wave_fn.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 3


def libm_is_the_tables_libm():
    """is this machine's libm the build csrc/tl_libm_tables.inc was read from (tests/test_libm_agree.py test_tables_are_this_libms_tables)?"""
    import hashlib
    inc = (ROOT / "odr-audioenc_amd" / "csrc" / "tl_libm_tables.inc").read_text()
    p = Path("/lib/x86_64-linux-gnu/libm.so.6")
    return p.exists() and hashlib.sha256(p.read_bytes()).hexdigest() in inc


def _ptr(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def run_libm(fn, form, table, a, b=None):
    """fn = probe_libm of the emulation or tlb_debug_probe_libm of the TEST library -> (rc, r0, r1)"""
    code, two_in, two_out, _ = FORMS[form]
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64) if two_in else None
    r0 = np.full(a.shape, np.nan)
    r1 = np.full(a.shape, np.nan) if two_out else None
    rc = fn(code, table, a.size, _ptr(a), _ptr(b), _ptr(r0), _ptr(r1))
    return rc, r0, r1


def run_wave(fn, prim, w_in, w_in2=None):
    """-> (rc, out): out uint64 [W, 64] ([W, 64, 4] for mirror4, [W, 64, 2] for ld2st2)"""
    w_in = np.ascontiguousarray(w_in, dtype=U64)
    w_in2 = np.ascontiguousarray(w_in2, dtype=U64) if prim in PRIM_TWO_IN else None
    W = w_in.shape[0]
    out = np.zeros((W, 64, 4) if prim == "mirror4" else (W, 64, 2) if prim == "ld2st2" else (W, 64), dtype=U64)
    rc = fn(PRIMS[prim], W, _ptr(w_in), _ptr(w_in2), _ptr(out))
    return rc, out


def same_bits(got, want):
    """bit for bit, NaN equal to NaN (tools/libm_agree.cpp same()) -> indices that differ"""
    g, w = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.flatnonzero((g.view(U64) != w.view(U64)) & ~(np.isnan(g) & np.isnan(w)))


# ------------------------------------------------------------------------------------------------------------------------------------
# arguments of the libm forms
def _u2d(u):
    return np.asarray(u, dtype=U64).view(np.float64)


def _d2u(d):
    return np.asarray(d, dtype=np.float64).view(U64)


class _Draw:
    def __init__(self, seed):
        self.r = np.random.default_rng(seed)

    def mant(self, n):                                                   # [1, 2), all 52 bits
        return _u2d(U64(0x3ff0000000000000) | self.r.integers(0, 1 << 52, n, dtype=U64))

    def binade(self, n, emin, emax):                                     # every binade emin..emax alike (subnormals below -1022)
        return np.ldexp(self.mant(n), self.r.integers(emin, emax + 1, n).astype(np.int32))

    def sign(self, n):
        return np.where(self.r.integers(0, 2, n) == 1, -1.0, 1.0)

    def uniform(self, n, lo, hi):                                        # (lo, hi): the ends themselves are edge-list matters
        return np.clip(self.r.uniform(lo, hi, n), np.nextafter(lo, hi), np.nextafter(hi, lo))

    def half(self, n):
        return np.where(self.r.integers(0, 2, n) == 1, 1.0, 0.5)

    def pick(self, n, parts):
        """parts: callables n -> array; argument i comes from part i % len(parts), as worker()'s switch (i % k)"""
        out = np.empty(n)
        for k, f in enumerate(parts):
            m = len(range(k, n, len(parts)))
            out[k::len(parts)] = f(m)
        return out


POW2_ALL = np.ldexp(1.0, np.arange(-1074, 1024, dtype=np.int32))
ONES = np.array([1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0)])
MINN, MAXN, MINSUB = float(np.ldexp(1.0, -1022)), float(np.finfo(np.float64).max), float(np.ldexp(1.0, -1074))
PI4 = 0.78539816339744830962


def _pow2(lo, hi):
    return POW2_ALL[(POW2_ALL >= lo) & (POW2_ALL <= hi)]


def _around(bits):
    return _u2d(np.array([bits - 1, bits, bits + 1], dtype=U64))


def _pm(x):
    x = np.asarray(x, dtype=np.float64)
    return np.concatenate([x, -x])


def _cross(ys, xs):
    g = np.array(np.meshgrid(ys, xs, indexing="ij")).reshape(2, -1)
    return g[0], g[1]


def _log_args(d, n):
    win = lambda m: _u2d(U64(0x3fee000000000000) + d.r.integers(0, 0x0003090000000000, m, dtype=U64) - U64(0x800) + d.r.integers(0, 0x1000, m, dtype=U64))
    rnd = d.pick(n, [lambda m: d.binade(m, -1022, 1023), lambda m: d.uniform(m, 0.9, 1.1), lambda m: d.mant(m) * d.half(m),
                     lambda m: d.uniform(m, 1e-20, 1e-10), lambda m: d.binade(m, -70, 40), lambda m: d.binade(m, -1022, -1000), win,
                     lambda m: np.maximum(d.uniform(m, 0.0, 70000.0 * 70000.0), MINN)])
    edge = np.concatenate([_pow2(MINN, MAXN), ONES, [1e-20, MINN, MAXN, 0.5, 2.0, 10.0], _around(0x3fee000000000000), _around(0x3ff1090000000000)])
    return np.concatenate([rnd, edge])


def _exp_args(d, n):
    top = np.nextafter(512.0, 0.0)
    rnd = d.pick(n, [lambda m: d.uniform(m, -512.0, 512.0), lambda m: d.uniform(m, -60.0, 5.0), lambda m: d.sign(m) * d.binade(m, -60, 8),
                     lambda m: d.uniform(m, -1.0, 1.0), lambda m: d.sign(m) * d.binade(m, -1074, -50), lambda m: d.uniform(m, -512.0, -500.0)])
    edge = _pm(np.concatenate([[0.0, 1e-20, MINSUB, MINN, top], _pow2(MINSUB, 256.0), ONES, _around(0x3c90000000000000)]))     # (2^-54: the 1 + x cut)
    return np.concatenate([rnd, edge])


def _pow10_args(d, n):
    top = np.nextafter(222.0, 0.0)
    rnd = d.pick(n, [lambda m: d.uniform(m, -222.0, 222.0), lambda m: d.uniform(m, -20.0, 20.0), lambda m: d.sign(m) * d.binade(m, -80, 6),
                     lambda m: d.sign(m) * d.uniform(m, 128.0, 222.0), lambda m: -0.1 * (d.r.integers(0, 4001, m) - 2000).astype(np.float64) * 0.1])
    edge = _pm(np.concatenate([[0.0, 1e-20, MINSUB, MINN, top], _pow2(MINSUB, 128.0), ONES, _around(0x3be0000000000000)]))     # (2^-65: the 1.0 cut)
    return np.concatenate([rnd, edge])


def _sincos_args(d, n):
    lim = 105414350.0
    near = lambda m: d.r.integers(0, 64, m).astype(np.float64) * PI4 * d.sign(m) + d.uniform(m, -1e-6, 1e-6) * d.r.integers(0, 2, m)
    rnd = d.pick(n, [lambda m: d.uniform(m, -12.0, 12.0), lambda m: d.uniform(m, -0.9, 0.9), lambda m: d.sign(m) * d.binade(m, -40, 25),
                     lambda m: d.uniform(m, -lim, lim), lambda m: d.sign(m) * d.uniform(m, 0.8, 2.5), near,
                     lambda m: d.sign(m) * (0.855469 + d.uniform(m, -1e-6, 1e-6)), lambda m: d.sign(m) * (2.426265 + d.uniform(m, -1e-6, 1e-6))])
    edge = _pm(np.concatenate([[0.0, 1e-20, MINSUB, MINN, np.nextafter(lim, 0.0), 0.126, np.nextafter(0.126, 0.0), np.nextafter(0.126, 1.0)],
                               _pow2(MINSUB, 2.0 ** 26), ONES, np.arange(64) * PI4,
                               _around(0x3feb600000000000), _around(0x400368fd00000000), _around(0x3e40000000000000)]))
    return np.concatenate([rnd, edge])


def _atan2_args(d, n):
    def c2(m):
        big, oth = d.sign(m) * d.binade(m, -443, 499), d.sign(m) * d.binade(m, -1022, 499)
        sw = d.r.integers(0, 2, m) == 1
        return np.where(sw, big, oth), np.where(sw, oth, big)

    def c3(m):
        x = d.sign(m) * d.binade(m, -20, 20)
        return x * d.uniform(m, -1.001, 1.001), x

    def c4(m):
        x = d.sign(m) * d.binade(m, -20, 20)
        return x * d.uniform(m, -0.07, 0.07), x

    def c5(m):
        y = d.sign(m) * d.binade(m, -20, 20)
        return y, y * d.uniform(m, -0.07, 0.07)

    def c7(m):
        z = lambda: np.where(d.r.integers(0, 16, m) == 0, 0.0 * d.sign(m), d.uniform(m, -3e4, 3e4) * d.r.random(m))
        return z(), z()

    parts = [lambda m: (d.sign(m) * d.binade(m, -40, 40), d.sign(m) * d.binade(m, -40, 40)), lambda m: (d.uniform(m, -1.0, 1.0), d.uniform(m, -1.0, 1.0)),
             c2, c3, c4, c5, lambda m: ((d.r.integers(0, 65536, m) - 32768).astype(np.float64), (d.r.integers(0, 65536, m) - 32768).astype(np.float64)), c7]
    y, x = np.empty(n), np.empty(n)
    for k, f in enumerate(parts):
        y[k::len(parts)], x[k::len(parts)] = f(len(range(k, n, len(parts))))
    x = np.where(np.maximum(np.abs(y), np.abs(x)) < 2.0 ** -443, 1.0, x)          # (0, 0) and the like lie outside the form's domain: x = 1 instead
    lo, hi = 2.0 ** -443, 2.0 ** 500
    vals = _pm([0.0, 1.0, ONES[1], ONES[2], 1e-20, lo, hi, MINSUB, MINN, 0.0625, np.nextafter(0.0625, 1.0), 3.0, 2.0 ** -57, 2.0 ** 57, 32768.0])
    ey, ex = _cross(vals, vals)
    big = np.maximum(np.abs(ey), np.abs(ex))
    ok = (big >= lo) & (big <= hi)
    return np.concatenate([y, ey[ok]]), np.concatenate([x, ex[ok]])


def _divns_args(d, n):
    """(dividend, divisor): divisor in [2^-500, 2^500], dividend +0 or of magnitude in [2^-900, 2^500], either sign"""
    def c(k):
        def f(m):
            if k == 0:
                return d.binade(m, -900, 499), d.binade(m, -500, 499)
            if k == 1:
                dv = d.uniform(m, 0.02, 4e7)
                return dv * d.uniform(m, 2.0 ** -57, 1.0), dv
            if k == 2:
                return d.mant(m) * d.half(m), d.mant(m)
            if k == 3:
                dv = d.binade(m, -5, 30)
                return dv * d.mant(m) * 2.0 ** -106, dv
            return np.where(d.r.integers(0, 64, m) == 0, 0.0, d.uniform(m, 0.0, 4e9)), d.uniform(m, 0.02, 4e9)
        return f
    nn, dd = np.empty(n), np.empty(n)
    for k in range(5):
        nn[k::5], dd[k::5] = c(k)(len(range(k, n, 5)))
    nn = np.where((d.r.integers(0, 4, n) == 0) & (nn != 0), -nn, nn)               # (the second quotient's dividend is a residual of either sign; a zero is +0)
    lo, hi = 2.0 ** -500, 2.0 ** 500
    en = np.concatenate([[0.0], _pm(np.concatenate([[1e-20, 2.0 ** -900, hi, 3.0], ONES, _pow2(2.0 ** -900, hi)[::37]]))])
    ed = np.concatenate([[1e-20, lo, hi, 3.0, 10.0], ONES, _pow2(lo, hi)[::41]])
    a, b = _cross(en, ed)
    return np.concatenate([nn, a]), np.concatenate([dd, b])


def _sqrtnz_args(d, n):
    lo, hi = 2.0 ** -500, 2.0 ** 500
    rnd = d.pick(n, [lambda m: d.binade(m, -500, 499), lambda m: d.uniform(m, 0.0005, 1e18), lambda m: d.mant(m) * (d.half(m) * 2.0)])
    return np.concatenate([rnd, _pow2(lo, hi), ONES, [1e-20, lo, hi, 0.0005, 2.0, 3.0, 4.0]])


def _div_args(d, n):
    a, b = _divns_args(d, n // 2)
    a, b = a[:n // 2], b[:n // 2] * d.sign(n // 2)
    m = n - n // 2
    a2, b2 = d.sign(m) * d.binade(m, -1074, 1023), d.sign(m) * d.binade(m, -1074, 1023)
    sp = _pm([0.0, np.inf, MINSUB, 123 * MINSUB, np.nextafter(MINN, 0.0), MINN, MAXN, 1.0, ONES[1], ONES[2], 1e-20, 3.0, 2.0 ** -900, 2.0 ** 500])
    sp = np.concatenate([sp, [np.nan]])
    ea, eb = _cross(sp, sp)
    return np.concatenate([a, a2, ea]), np.concatenate([b, b2, eb])


def _sqrt_args(d, n):
    rnd = d.pick(n, [lambda m: d.binade(m, -1074, 1023), lambda m: d.binade(m, -500, 499), lambda m: d.uniform(m, 0.0005, 1e18),
                     lambda m: d.mant(m) * (d.half(m) * 2.0), lambda m: d.binade(m, -1074, -1000), lambda m: -d.binade(m, -1074, 1023)])
    return np.concatenate([rnd, POW2_ALL, ONES, _pm([0.0, np.inf, MINSUB, 123 * MINSUB, np.nextafter(MINN, 0.0), MINN, MAXN, 1e-20, 1.0, 2.0, 3.0, 4.0]), [np.nan]])


def _minmax_args(d, n):
    """neither a NaN; zeros of OPPOSITE sign are the primitive's documented exception (signed_zero_ties) and not in this set"""
    a = d.pick(n, [lambda m: d.sign(m) * d.binade(m, -1074, 1023), lambda m: d.uniform(m, -100.0, 100.0), lambda m: d.binade(m, -30, 30), lambda m: d.uniform(m, 0.0, 1.0)])
    b = d.pick(n, [lambda m: d.sign(m) * d.binade(m, -1074, 1023), lambda m: d.uniform(m, -100.0, 100.0), lambda m: d.binade(m, -30, 30), lambda m: np.full(m, 0.0005)])
    b[7::8] = a[7::8]                                                     # ties
    sp = _pm([np.inf, MINSUB, MINN, MAXN, 1.0, ONES[1], 1e-20, 0.0005])
    ea, eb = _cross(sp, sp)
    z = np.array([0.0, 0.0, -0.0, -0.0, 0.0, -0.0, 1.0, -1.0]), np.array([0.0, 1.0, -0.0, -1.0, -1.0, 1.0, 0.0, -0.0])       # zeros of ONE sign, zeros against others
    return np.concatenate([a, ea, z[0]]), np.concatenate([b, eb, z[1]])


def _fmak_args(d, n):
    def cancel(m):                                                        # a b close to -K: the sum's leading bits cancel, the fused product's low half decides
        a = d.sign(m) * d.uniform(m, 0.25, 4.0)
        return a, -FMA_K / a * (1.0 + d.uniform(m, -2.0 ** -40, 2.0 ** -40))
    parts = [lambda m: (d.sign(m) * d.binade(m, -30, 30), d.sign(m) * d.binade(m, -30, 30)), lambda m: (d.uniform(m, -1.0, 1.0), d.uniform(m, 0.0, 1.0)), cancel,
             lambda m: (d.sign(m) * d.binade(m, -1074, 1000), d.sign(m) * d.binade(m, -1074, 20))]
    a, b = np.empty(n), np.empty(n)
    for k, f in enumerate(parts):
        a[k::4], b[k::4] = f(len(range(k, n, 4)))
    sp = _pm([0.0, 1.0, ONES[1], 1e-20, MINSUB, MINN, 2.0 ** 500, -FMA_K, 3.0])
    ea, eb = _cross(sp, sp)
    return np.concatenate([a, ea]), np.concatenate([b, eb])


_args = {}


def arguments(form):
    """-> (a, b or None): the form's full argument set, the same arrays on every call"""
    if form not in _args:
        d = _Draw(20260000 + FORMS[form][0])
        n = NRANDOM
        if form in ("log_pn", "log10_pn", "log10_split"):
            r = _log_args(d, n), None
        elif form == "exp_sl":
            r = _exp_args(d, n), None
        elif form == "pow10_sl":
            r = _pow10_args(d, n), None
        elif form in ("sincos_sl", "sincos_phased"):
            r = _sincos_args(d, n), None
        elif form == "sincos_phased_raw":
            a = _sincos_args(d, n)
            r = a, d.r.permutation(_sincos_args(d, n))
        elif form in ("atan2_phased", "atan2_ns"):
            r = _atan2_args(d, n)
        elif form == "div_ns":
            r = _divns_args(d, n)
        elif form == "sqrt_ns":
            r = np.concatenate([_sqrtnz_args(d, n), [0.0, -0.0]]), None
        elif form in ("sqrt_nz", "rsq_seed"):
            r = _sqrtnz_args(d, n), None
        elif form in ("rcp_seed", "recip"):
            r = _divns_args(d, n)[1], None
        elif form == "div":
            r = _div_args(d, n)
        elif form == "sqrt":
            r = _sqrt_args(d, n), None
        elif form in ("min_nn", "max_nn"):
            r = _minmax_args(d, n)
        else:
            r = _fmak_args(d, n)
        for x in r:
            if x is not None:
                x.setflags(write=False)
        _args[form] = r
    return _args[form]


def sincos_quadrant_is_odd(x):
    """csrc/tl_libm.h, the comment above tlm_sincos_reduce: quadrant 0 for |x| < 0.85546875, 1 / 3 up to 2.426265, else the low bits of
    x / (pi / 2) rounded to an integer (two single IEEE operations, as numpy evaluates them)"""
    k = (_d2u(x) >> U64(32)).astype(np.int64) & 0x7fffffff
    t = x * float(_u2d([0x3fe45f306dc9c883])[0]) + float(_u2d([0x4338000000000000])[0])
    n = (_d2u(t) & U64(1)).astype(np.int64)
    return np.where(k < 0x3feb6000, 0, np.where(k < 0x400368fd, 1, n)) == 1


_want = {}


def glibc(form):
    """this machine's libm on arguments(form) -> (r0, r1 or None), computed once"""
    if form in _want:
        return _want[form]
    R = ref()
    a, b = arguments(form)
    a = np.ascontiguousarray(a)
    b = None if b is None else np.ascontiguousarray(b)
    n = a.size
    r0, r1 = np.empty(n), None
    one = lambda f, x: (f(n, _ptr(x), _ptr(r0)), r0)[1]
    if form == "log_pn":
        one(R.ref_log, a)
    elif form in ("log10_pn", "log10_split"):
        one(R.ref_log10, a)
    elif form == "pow10_sl":
        one(R.ref_pow10, a)
    elif form == "exp_sl":
        one(R.ref_exp, a)
    elif form in ("sincos_sl", "sincos_phased", "sincos_phased_raw"):
        r1 = np.empty(n)
        R.ref_sincos(n, _ptr(a), _ptr(r0), _ptr(r1))
        if form == "sincos_phased_raw":                                   # the pair arrives exchanged where the OTHER phase's quadrant is odd
            odd = sincos_quadrant_is_odd(b)
            r0, r1 = np.where(odd, r1, r0), np.where(odd, r0, r1)
    elif form in ("atan2_phased", "atan2_ns"):
        R.ref_atan2(n, _ptr(a), _ptr(b), _ptr(r0))
    elif form in ("div_ns", "div"):
        R.ref_div(n, _ptr(a), _ptr(b), _ptr(r0))
    elif form in ("sqrt_ns", "sqrt_nz", "sqrt"):
        one(R.ref_sqrt, a)
    elif form in ("rcp_seed", "recip"):                                   # (the HOST half's seed: the exact reciprocal, rounded; the refined one has no libm counterpart)
        R.ref_div(n, _ptr(np.ones(n)), _ptr(a), _ptr(r0))
    elif form == "rsq_seed":
        s = np.empty(n)
        R.ref_sqrt(n, _ptr(a), _ptr(s))
        R.ref_div(n, _ptr(np.ones(n)), _ptr(s), _ptr(r0))
    elif form == "min_nn":
        r0 = np.where(b < a, b, a)
    elif form == "max_nn":
        r0 = np.where(a < b, b, a)
    else:
        assert form == "fma_k"
        R.ref_fma(n, _ptr(a), _ptr(b), FMA_K, _ptr(r0))
    _want[form] = (r0, r1)
    return _want[form]


def seed_error(form, x, seed):
    """the largest relative error of the seeds (and of the refined reciprocal): max |seed d - 1| resp. max |seed^2 x - 1| / 2, in 64-bit-mantissa
    arithmetic (the product of two doubles rounded once more: error < 2^-63)"""
    assert np.finfo(np.longdouble).nmant >= 63
    xl, sl = x.astype(np.longdouble), seed.astype(np.longdouble)
    e = np.abs(sl * xl - 1) if form in ("rcp_seed", "recip") else np.abs(sl * sl * xl - 1) / 2
    return float(e.max())


# ------------------------------------------------------------------------------------------------------------------------------------
# cases and oracles of the wave primitives
def _i32_words(v):
    return np.asarray(v, dtype=np.int64).astype(U64)                       # sign-extended; the body reads the low half


def _put(base, lane, val):
    w = base.copy()
    w[lane] = val
    return w


def _key_cases(r):
    big = lambda: r.integers(1 << 62, 1 << 63, 64, dtype=U64)
    rnd = [r.integers(0, 1 << 64, (NWAVES // 4, 64), dtype=U64, endpoint=False),
           r.integers(0, 5, (NWAVES // 4, 64), dtype=U64) << U64(32) | r.integers(0, 1 << 32, (NWAVES // 4, 64), dtype=U64),      # high words tie, low decide
           r.integers(0, 1 << 32, (NWAVES // 4, 64), dtype=U64) << U64(32) | r.integers(0, 3, (NWAVES // 4, 64), dtype=U64),      # ... and the reverse
           np.where(r.integers(0, 4, (NWAVES // 4, 64)) == 0, r.integers(0, 4, (NWAVES // 4, 64), dtype=U64), ALL1)]              # few live keys, many ties, ~0 elsewhere
    rnd[3][::7] |= U64(0xffffffff00000000)                                # live keys whose high word is all ones
    made = []
    for p in SPECIAL_LANES:
        b = big()
        made += [_put(b, p, U64(5)),                                                           # the smallest key in lane p
                 _put(np.full(64, (U64(9) << U64(32)) | U64(1000), dtype=U64), p, (U64(9) << U64(32)) | U64(7)),       # high words tie, the low word decides
                 _put(np.full(64, (U64(9) << U64(32)) | U64(7), dtype=U64), p, (U64(8) << U64(32)) | U64(7)),          # low words tie, the high word decides
                 _put(np.full(64, ALL1, dtype=U64), p, U64(0xffffffff00000005)),                                       # one live key, its high word all ones
                 _put(np.full(64, ALL1, dtype=U64), p, U64(3))]
    made += [np.full(64, U64(77), dtype=U64), np.full(64, ALL1, dtype=U64), np.zeros(64, dtype=U64)]
    for odd, even in ((15, 48), (1, 2), (1, 62), (31, 32), (61, 62), (47, 48)):                # a tie between an odd lane below and an even lane above
        b = big()
        b[odd] = b[even] = U64(11)
        made.append(b)
        hi = np.full(64, (U64(4) << U64(32)) | U64(900), dtype=U64)                            # ... whose high words tie with everyone's
        hi[odd] = hi[even] = (U64(4) << U64(32)) | U64(2)
        made.append(hi)
    for lanes in ((15, 47), (1, 63), (63, 1, 33), (17, 15)):                                   # ties on odd lanes only
        b = big()
        b[list(lanes)] = U64(11)
        made.append(b)
    for lanes in ((15, 48), (0, 63), (14, 17)):                                                # the minimum's high word in one lane pair, its low word decides
        b = np.full(64, (U64(6) << U64(32)) | U64(50), dtype=U64)
        b[lanes[0]] = (U64(2) << U64(32)) | U64(40)
        b[lanes[1]] = (U64(2) << U64(32)) | U64(30)
        made.append(b)
    return np.concatenate(rnd + [np.array(made, dtype=U64)])


def _i32_cases(r):
    lim = 1 << 24                                                         # no 64-term sum overflows (signed overflow is undefined in the emulation)
    rnd = r.integers(-lim, lim + 1, (NWAVES, 64))
    made = [np.full(64, 0x7fffffff >> 6), np.full(64, -lim), np.full(64, lim), np.zeros(64, dtype=np.int64), -np.abs(rnd[0]) - 1, np.arange(64), -np.arange(64)]
    for p in SPECIAL_LANES:
        made += [_put(np.zeros(64, dtype=np.int64), p, -lim), _put(np.full(64, -3), p, lim)]
    return _i32_words(np.concatenate([rnd, np.array(made)]))


def _u32_cases(r):
    rnd = r.integers(0, 1 << 32, (NWAVES, 64), dtype=U64)
    made = [np.zeros(64, dtype=U64), np.full(64, 0xffffffff, dtype=U64)] + [_put(np.zeros(64, dtype=U64), p, U64(0x80000001)) for p in SPECIAL_LANES]
    return np.concatenate([rnd, np.array(made, dtype=U64)])


def _f64_value_cases(r):
    """numbers (no NaN: no caller of the row maximum makes one): dB-like values, all binades, negatives only, infinities, ties, zeros"""
    rnd = [r.normal(0.0, 60.0, (NWAVES // 2, 64)), np.ldexp(r.uniform(1.0, 2.0, (NWAVES // 4, 64)), r.integers(-1074, 1024, (NWAVES // 4, 64)).astype(np.int32)) * r.choice([-1.0, 1.0], (NWAVES // 4, 64)),
           np.round(r.normal(0.0, 2.0, (NWAVES // 4, 64)))]                                      # few distinct values: ties, +0.0 among them
    made = [-np.abs(rnd[0][0]) - 1.0, np.full(64, -np.inf), np.full(64, np.inf), np.full(64, 3.25), np.full(64, -3.25), np.zeros(64), np.full(64, -0.0),
            np.tile([-0.0, 0.0], 32), np.tile([0.0, -0.0], 32), np.tile([-0.0] * 8 + [0.0] * 8, 4), np.tile([0.0] * 8 + [-0.0] * 8, 4),
            np.tile([-0.0] + [-1.0] * 14 + [0.0], 4), np.tile([0.0] + [-1.0] * 14 + [-0.0], 4)]
    for p in SPECIAL_LANES:
        b = r.normal(0.0, 60.0, 64)
        made += [_put(b, p, 1e6), _put(b, p, np.inf), _put(np.full(64, -np.inf), p, -1e300), _put(-np.abs(b) - 1.0, p, -0.5)]
    return np.concatenate(rnd + [np.array(made)]).view(U64)


def _bits_cases(r, shape_tail=()):
    rnd = r.integers(0, 1 << 64, (NWAVES,) + (64,) + shape_tail, dtype=U64, endpoint=False)
    lanes = np.broadcast_to(np.arange(64, dtype=U64).reshape((64,) + (1,) * len(shape_tail)), (64,) + shape_tail)
    made = [lanes * U64(0x0101010101010101) + U64(1), np.zeros((64,) + shape_tail, dtype=U64), np.full((64,) + shape_tail, ALL1, dtype=U64)]
    return np.concatenate([rnd, np.array(made, dtype=U64)])


def _mask_cases(r):
    masks = [0, 0xffffffffffffffff, 1 << 63, 1, 0x5555555555555555, 0xaaaaaaaaaaaaaaaa, 0xffffffff00000000, 0x00000000ffffffff, 0x8000000000000001, 1 << 31, 1 << 32]
    masks += [1 << p for p in SPECIAL_LANES] + [0xffffffffffffffff ^ (1 << p) for p in SPECIAL_LANES]
    masks += [int(x) for x in r.integers(0, 1 << 64, NWAVES, dtype=U64, endpoint=False)]
    bits = (np.array(masks, dtype=U64)[:, None] >> np.arange(64, dtype=U64)[None, :]) & U64(1)
    live = r.choice(np.array([1, 1 << 32, 1 << 63, 0xffffffff00000000, 0x12345], dtype=U64), bits.shape)      # "not zero" in either half of the word
    return np.where(bits == 1, live, U64(0))


_cases = {}


def wave_cases(prim):
    """-> (in, in2 or None), the same arrays on every call"""
    if prim in _cases:
        return _cases[prim]
    r = np.random.default_rng(20261000 + PRIMS[prim])
    in2 = None
    if prim in ("wave_min_u64", "wave_argmin_u64", "par_min_u64", "swap1_u64"):
        w = _key_cases(r)
    elif prim in ("wave_sum_i32", "wave_exscan_i32", "par_sum_i32"):
        w = _i32_cases(r)
    elif prim in ("wave_xor_u32", "wave_incl_xscan_u32"):
        w = _u32_cases(r)
    elif prim == "row16_max_f64":
        w = _f64_value_cases(r)
    elif prim in ("ballot", "rank_below"):
        w = _mask_cases(r)
    elif prim in ("swap1_f64", "rot32_f64", "mirror1"):
        w = _bits_cases(r)
    elif prim == "mirror4":
        w = _bits_cases(r, (4,))
    elif prim == "other":
        w = _bits_cases(r)
        in2 = r.integers(0, 64, w.shape, dtype=U64)
        in2[0], in2[1], in2[2], in2[3] = np.arange(64), 63 - np.arange(64), 63, 0          # identity, reversal, all from lane 63, all from lane 0
    elif prim == "readlane_i32":
        w = _i32_cases(r)
        in2 = np.repeat(r.integers(0, 64, (w.shape[0], 1), dtype=U64), 64, axis=1)
        for k, p in enumerate(SPECIAL_LANES):
            in2[k] = p
    elif prim == "uni_i":
        v = np.concatenate([r.integers(-(1 << 31), 1 << 31, NWAVES), [0, -1, 0x7fffffff, -(1 << 31)]])
        w = _i32_words(np.repeat(v[:, None], 64, axis=1))
    elif prim == "select":
        w = _bits_cases(r)
        in2 = _mask_cases(r)[:w.shape[0]]
    elif prim == "sign_bit":
        sp = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, MINSUB, -MINSUB, MAXN, -MAXN, 1e-20, -1e-20], dtype=np.float64).view(U64)
        w = np.concatenate([_bits_cases(r), _f64_value_cases(r)[:512], np.resize(sp, (2, 64)),
                            np.resize(np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0xfff0000000000001], dtype=U64), (1, 64))])
    else:
        assert prim == "ld2st2"
        w = _bits_cases(r)
        in2 = r.permutation(_bits_cases(r))
    for x in (w, in2):
        if x is not None:
            x.setflags(write=False)
    _cases[prim] = (w, in2)
    return _cases[prim]


def _sx32(v):
    """the low 32 bits as a signed number, sign-extended into the word"""
    return ((np.asarray(v).astype(np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)).astype(U64)


def _lo32(w):
    return ((w & U64(0xffffffff)).astype(np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)


def wave_oracle(prim, w, in2=None):
    """what the primitive means (the comments of csrc/mp2_wave.h) -> (expected out, lanes compared: bool [64])"""
    W = w.shape[0]
    lanes = np.arange(64)
    every = np.ones(64, dtype=bool)
    bc = lambda v: np.repeat(np.asarray(v)[:, None], 64, axis=1)
    if prim == "wave_min_u64":
        return bc(w.min(axis=1)), every
    if prim == "wave_argmin_u64":
        out = np.empty(W, dtype=np.int64)
        for i in range(W):                                                # the smallest key; ties: even lanes first, then ascending; -1 when every key is ~0
            m = min(int(k) for k in w[i])
            at = [l for l in range(64) if int(w[i, l]) == m]
            ev = [l for l in at if l % 2 == 0]
            out[i] = -1 if m == 0xffffffffffffffff else (ev[0] if ev else at[0])
        return bc(out.astype(U64)), every
    if prim == "wave_sum_i32":
        return bc(_sx32(_lo32(w).sum(axis=1))), every
    if prim == "wave_xor_u32":
        return bc(np.bitwise_xor.reduce(w & U64(0xffffffff), axis=1)), every
    if prim == "wave_exscan_i32":
        v = _lo32(w)
        return _sx32(np.cumsum(v, axis=1) - v), every
    if prim == "wave_incl_xscan_u32":
        return np.bitwise_xor.accumulate(w & U64(0xffffffff), axis=1), every
    if prim == "row16_max_f64":                                           # the row's maximum, of tied maxima the last (its bits: -0.0 and +0.0 tie); lane 15 of each row
        v = w.view(np.float64).reshape(W, 4, 16)
        tied = v == v.max(axis=2, keepdims=True)
        last = 15 - np.argmax(tied[:, :, ::-1], axis=2)
        m = np.take_along_axis(w.reshape(W, 4, 16), last[:, :, None], axis=2)
        return np.repeat(m, 16, axis=2).reshape(W, 64), lanes % 16 == 15
    if prim == "par_min_u64":                                             # over the lanes of the caller's parity
        out = np.empty_like(w)
        out[:, 0::2] = w[:, 0::2].min(axis=1, keepdims=True)
        out[:, 1::2] = w[:, 1::2].min(axis=1, keepdims=True)
        return out, every
    if prim == "par_sum_i32":
        v = _lo32(w)
        out = np.empty((W, 64), dtype=np.int64)
        out[:, 0::2] = v[:, 0::2].sum(axis=1, keepdims=True)
        out[:, 1::2] = v[:, 1::2].sum(axis=1, keepdims=True)
        return _sx32(out), every
    if prim in ("ballot", "rank_below"):
        bits = (w != 0).astype(U64)
        if prim == "ballot":
            return bc((bits << np.arange(64, dtype=U64)[None, :]).sum(axis=1, dtype=U64)), every
        return (np.cumsum(bits, axis=1, dtype=U64) - bits), every         # set bits below the lane
    if prim in ("swap1_u64", "swap1_f64"):
        return w[:, lanes ^ 1], every
    if prim == "rot32_f64":
        return w[:, (lanes + 32) & 63], every
    if prim in ("mirror1", "mirror4"):                                    # the lane of subband 31 - sb of the same channel
        return w[:, 2 * (31 - (lanes >> 1)) + (lanes & 1)], every
    if prim == "other":
        return np.take_along_axis(w, in2.astype(np.int64), axis=1), every
    if prim == "readlane_i32":
        return bc(_sx32(_lo32(w)[np.arange(W), in2[:, 0].astype(np.int64)])), every
    if prim == "uni_i":
        return _sx32(_lo32(w)), every
    if prim == "select":
        return np.where(in2 != 0, w, ~w), every
    if prim == "sign_bit":
        return w >> U64(63), every
    assert prim == "ld2st2"
    return np.stack([w[:, ::-1], in2[:, ::-1]], axis=2), every


# zeros of opposite sign: the one input on which TLM_MIN_NN / TLM_MAX_NN's halves differ, outside the macros' stated precondition (csrc/tl_libm.h)
SIGNED_ZERO_TIES = (np.array([0.0, -0.0]), np.array([-0.0, 0.0]))


# ------------------------------------------------------------------------------------------------------------------------------------
# what both test files share
LIBM_FORMS = [(f, t) for f, spec in FORMS.items() for t in spec[3]]


def report(form, a, b, got, want, bad):
    i = bad[0]
    return "%s: %d of %d differ; first: a=%r b=%r got %r want %r" % (form, bad.size, a.size, float(a[i]).hex(), None if b is None else float(b[i]).hex(),
                                                                      float(got[i]).hex(), float(want[i]).hex())


OUTSIDE = {
    "log_pn": [0.0, -1.0, 5e-324, np.inf, np.nan], "log10_pn": [0.0, -1.0, 5e-324, np.inf, np.nan], "log10_split": [2.0 ** -1023, np.nan],
    "pow10_sl": [222.0, -222.0, np.inf, np.nan], "exp_sl": [512.0, -512.0, -np.inf, np.nan],
    "sincos_sl": [105414350.0, -105414350.0, 1e300, np.inf, np.nan], "sincos_phased": [105414350.0, -1e10, np.inf, np.nan],
    "sqrt_ns": [-1.0, 2.0 ** -501, 2.0 ** 501, np.inf, np.nan, 5e-324], "sqrt_nz": [0.0, -0.0, 2.0 ** -501, 2.0 ** 501, np.nan],
    "rcp_seed": [0.0, -1.0, 2.0 ** 501, np.nan], "rsq_seed": [0.0, -1.0, 2.0 ** -501, np.inf],
}
OUTSIDE2 = {
    "sincos_phased_raw": [(1.0, 105414350.0), (np.nan, 1.0), (1e9, 0.0)],
    "atan2_phased": [(0.0, 0.0), (2.0 ** -444, 2.0 ** -444), (2.0 ** 501, 1.0), (1.0, np.inf), (np.nan, 1.0), (1.0, np.nan)],
    "atan2_ns": [(0.0, -0.0), (2.0 ** -444, 0.0), (1.0, 2.0 ** 501), (np.inf, np.inf), (np.nan, np.nan)],
    "div_ns": [(-0.0, 1.0), (1.0, 0.0), (1.0, -1.0), (1.0, 2.0 ** -501), (1.0, 2.0 ** 501), (2.0 ** -901, 1.0), (2.0 ** 501, 1.0), (np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0)],
    "min_nn": [(np.nan, 1.0), (1.0, np.nan)], "max_nn": [(np.nan, 1.0), (1.0, np.nan)], "fma_k": [(np.inf, 1.0), (1.0, np.nan)],
}


def check_argument_checks(libm_fn, wave_fn):
    """what the probe refuses with TLB_ERR_ARG, the same for the emulation's entry and the device's (both test files call this):
    an argument outside the form's domain -- alone, or last among good ones --, an unknown form, n = 0, a missing pointer"""
    good = np.array([1.5, 2.5, 3.5])
    for form, xs in OUTSIDE.items():
        for x in xs:
            assert run_libm(libm_fn, form, 0, np.array([x]))[0] == ERR_ARG, (form, x)
            assert run_libm(libm_fn, form, 0, np.append(good, x))[0] == ERR_ARG, (form, x)
    for form, ps in OUTSIDE2.items():
        for a, b in ps:
            assert run_libm(libm_fn, form, 0, np.append(good, a), np.append(good, b))[0] == ERR_ARG, (form, a, b)
    buf = np.ones(4)
    p = buf.ctypes.data_as(C.c_void_p)
    assert libm_fn(-1, 0, 4, p, p, p, p) == ERR_ARG and libm_fn(NFORMS, 0, 4, p, p, p, p) == ERR_ARG
    assert libm_fn(0, 0, 0, p, p, p, p) == ERR_ARG and libm_fn(0, 0, -4, p, p, p, p) == ERR_ARG
    assert libm_fn(0, 2, 4, p, p, p, p) == ERR_ARG and libm_fn(FORMS["exp_sl"][0], 1, 4, p, p, p, p) == ERR_ARG      # a table placement the form has not
    assert libm_fn(0, 0, 4, None, p, p, p) == ERR_ARG and libm_fn(0, 0, 4, p, p, None, p) == ERR_ARG
    assert libm_fn(FORMS["div_ns"][0], 0, 4, p, None, p, p) == ERR_ARG and libm_fn(FORMS["sincos_sl"][0], 0, 4, p, p, p, None) == ERR_ARG
    w = np.zeros((2, 64), dtype=np.uint64)
    q = w.ctypes.data_as(C.c_void_p)
    assert wave_fn(-1, 2, q, q, q) == ERR_ARG and wave_fn(NPRIMS, 2, q, q, q) == ERR_ARG and wave_fn(0, 0, q, q, q) == ERR_ARG
    assert wave_fn(0, 2, None, q, q) == ERR_ARG and wave_fn(0, 2, q, q, None) == ERR_ARG and wave_fn(PRIMS["other"], 2, q, None, q) == ERR_ARG
    lane = np.zeros((2, 64), dtype=np.uint64)
    lane[1, 63] = 64                                                      # not a lane number
    assert run_wave(wave_fn, "other", w, lane)[0] == ERR_ARG
    lane[1, 63], lane[1, 0] = 0, 1 << 40
    assert run_wave(wave_fn, "readlane_i32", w, lane)[0] == ERR_ARG
    uni = np.zeros((2, 64), dtype=np.uint64)
    uni[1, 17] = 1                                                        # TL_UNI_I's value is uniform by the caller's construction
    assert run_wave(wave_fn, "uni_i", uni)[0] == ERR_ARG
    # ... and a good call after all that returns the right bits
    rc, r0, _ = run_libm(libm_fn, "sqrt_nz", 0, np.array([4.0, 2.25, 1e10]))
    assert rc == 0 and r0.tolist() == [2.0, 1.5, 1e5]
    rc, out = run_wave(wave_fn, "wave_min_u64", np.arange(128, dtype=np.uint64).reshape(2, 64) + np.uint64(5))
    assert rc == 0 and (out[0] == 5).all() and (out[1] == 69).all()
