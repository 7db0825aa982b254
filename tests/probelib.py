"""Support for tests/test_probe_emu.py and tests/test_probe_gpu.py: the argument sets, the references and the bindings of the probe
(csrc/mp2_probe.h: every device-path form of csrc/tl_libm.h and every cross-lane primitive of csrc/mp2_wave.h, one by one; csrc/mp2_probe_stage.h:
every shared stage helper of csrc/mp2_dbsum.h and, one layer up, the bit allocation of csrc/mp2_alloc.h alone -- its sets and oracles are the last
part of this file).

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
    """tests/emu/mp2_probe_emu.cpp with the library's table builder (csrc/mp2_host.cpp), the flags of the other emulations (tests/loudnesslib.py GXX)"""
    L = _build("libmp2probeemu.so", GXX + ["-shared", str(ROOT / "tests" / "emu" / "mp2_probe_emu.cpp"), str(ROOT / "odr-audioenc_amd" / "csrc" / "mp2_host.cpp"), "-lm"])
    bind_probe(L.probe_libm, L.probe_wave)
    bind_stage(L.probe_stage)
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


def check_argument_checks(libm_fn, wave_fn, stage_fn):
    """what the probe refuses with TLB_ERR_ARG, the same for the emulation's entry and the device's (both test files call this):
    an argument outside the form's domain -- alone, or last among good ones --, an unknown form, n = 0, a missing pointer"""
    check_stage_argument_checks(stage_fn)
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


# ------------------------------------------------------------------------------------------------------------------------------------
# The third family: the stage helpers of csrc/mp2_dbsum.h (csrc/mp2_probe_stage.h).  Argument sets (fixed seeds) and oracles.  The oracles are
# written from what the comments of mp2_dbsum.h state, in the branchy shape of the model's description; the assertions are on raw bits and
# integers, nothing has a tolerance.  Tables (the dB-sum table, the scalefactors, the bark rows) are data read through the emulation library.
STAGE = {"add_db": 0, "mask": 1, "mnr_key": 2, "sf_index": 3, "div_by": 4, "spans": 5, "min_rows": 6, "bits": 7, "alloc": 8}
STAGE_NFORMS = 9
STAGE_TESTS = ("add_db", "mask", "spans", "min_rows", "mnr_key", "sf_index", "div_by", "put_bits", "put_bits48", "alloc", "alloc_pair")
NSTAGE_RANDOM = 1 << 18
TL_DBMIN = -200.0
FAR_HI = 0xC0F00000
MASKER_MAX, LIST, ROWS, FIELDS, FRAME_WORDS, FRAME_BITS = 128, 192, 136, 6, 434, 1728 * 8
RATES6 = (48000, 44100, 32000, 24000, 22050, 16000)
I32 = np.int32


def bind_stage(fn):
    fn.argtypes = [C.c_int, C.c_long] + [C.c_void_p] * 5


def _emu_tables():
    """the library's own tables through the emulation: dblog[0..1001], the scalefactors, the bark rows of psy 1 and psy 3 at the six rates"""
    if "tables" not in _built:
        L = emu()
        db, sf = np.empty(1002), np.empty(64)
        L.probe_dbtable(_ptr(db))
        L.probe_scalefactors(_ptr(sf))
        barks = {}
        for psy in (1, 3):
            for fs in RATES6:
                buf = np.empty(136)
                L.probe_bark_table.argtypes = [C.c_int, C.c_long, C.c_void_p]
                n = L.probe_bark_table(psy, fs, _ptr(buf))
                assert n > 100, (psy, fs, n)
                barks[(psy, fs)] = buf[:n].copy()
        _built["tables"] = (db, sf, barks)
    return _built["tables"]


def _near(x, k):
    """x and its k neighbours on either side"""
    out = [np.asarray(x, dtype=np.float64)]
    lo = hi = out[0]
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate([np.ravel(v) for v in out])


def _bits_report(name, what, i, args, got, want):
    h = lambda v: hex(int(np.asarray(v).view(U64 if np.asarray(v).dtype.itemsize == 8 else np.uint32))) if np.asarray(v).dtype.kind == "f" else hex(int(v))
    return "%s, %s: argument %d = %s -> %s, want %s" % (name, what, i, ", ".join("%s=%s" % (k, (float(v).hex() if isinstance(v, float) else v)) for k, v in args.items()), h(got), h(want))


# ---- 1. dB sums
def add_db_oracle(a, b, tab):
    """psycho_1.c:180-205 as the comment of tl_add_db states it: the larger operand beyond +-990, else the operand chosen by the sign of the
    truncated index plus the table entry"""
    f = 10.0 * (a - b)
    i = np.trunc(np.clip(f, -991.0, 991.0)).astype(np.int64)
    mid = np.where(i >= 0, a + tab[np.clip(i, 0, 990)], b + tab[np.clip(-i, 0, 990)])
    return np.where(f > 990.0, a, np.where(f < -990.0, b, mid))


def far_levels(n, seed=5):
    """levels whose high word is 0xC0F00000: what a masking term out of reach becomes"""
    r = np.random.default_rng(seed)
    lo = np.concatenate([[0, 1, 0xffffffff, 0x80000000], r.integers(0, 1 << 32, n - 4, dtype=U64)]).astype(U64)
    return _u2d((U64(FAR_HI) << U64(32)) | lo)


def add_db_set():
    """-> dict(a, b, named: {name: slice}, far: indices where one operand is the far level (the sum must be the other operand's bits))"""
    if "add_db" in _args:
        return _args["add_db"]
    A, B, named = [], [], {}

    def add(name, a, b):
        a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
        s = sum(len(x) for x in A)
        A.append(np.ravel(a).copy()); B.append(np.ravel(b).copy())
        named[name] = slice(s, s + a.size)

    lev = np.arange(-2000, 1201) / 10.0                                    # -200 .. 120
    add("equal operands", lev, lev)
    add("b = TL_DBMIN", lev, TL_DBMIN)
    add("a = TL_DBMIN", TL_DBMIN, lev)
    d = np.concatenate([_near(k / 10.0, 4) for k in range(-991, 992)])     # 10 (a - b): every integer in [-991, 991] and the doubles on both sides of it
    add("10 (a - b) at every integer, a - 0", d, 0.0)
    add("10 (a - b) at every integer, 0 - b", 0.0, -d)
    f = 10.0 * d
    ks = np.arange(-991, 992)
    assert np.isin(ks[np.abs(ks) % 2 == 0], f).mean() > 0.9 and all(np.isin([-991.0, -990.0, -1.0, 0.0, 1.0, 990.0, 991.0], f))
    for k in (-990, -1, 1, 990):                                           # ... each cut has arguments strictly on both sides
        assert (f[(f > k - 1e-9) & (f < k)].size and f[(f > k) & (f < k + 1e-9)].size)
    g = np.random.default_rng(41)
    i, j = g.integers(-2000, 1201, 20000), g.integers(-1000, 1001, 20000)
    add("0.1 dB grid", i * 0.1, np.clip(i - j, -2000, 1200) * 0.1)
    far = far_levels(512)
    other = np.resize(np.concatenate([[TL_DBMIN, -100.0, -0.0625, 0.0, -0.0, 15.0, 40.0, 96.3, 110.0], lev[::97]]), 512)
    add("far level as b", other, far)
    add("far level as a", far, other)
    z = np.array([0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.05, 0.05, -0.05, -0.05, 0.0, -0.0, 0.0, -0.0])
    zb = np.array([0.0, -0.0, -0.0, 0.0, 0.05, 0.05, 0.0, -0.0, 0.0, -0.0, -0.05, -0.05, 99.5, -99.5])
    add("signed zeros", z, zb)
    d99 = np.concatenate([_near(99.0, 4), _near(-99.0, 4)])
    for x in (-120.5, -50.25, 0.0, 60.125):
        add("differences around 99 dB at %g" % x, x, x - d99)
        add("differences around 99 dB below %g" % x, x - d99, x)
    nmade = sum(len(x) for x in A)
    add("random", g.uniform(-200.0, 120.0, NSTAGE_RANDOM), g.uniform(-200.0, 120.0, NSTAGE_RANDOM))
    S = dict(a=np.concatenate(A), b=np.concatenate(B), named=named, constructed=nmade, random=NSTAGE_RANDOM)
    S["far"] = (named["far level as b"], named["far level as a"])
    _args["add_db"] = S
    return S


def add_db_check(S, out0, out1, tab=None, ref=None):
    """out0 / out1 of a run against the oracle (tab) or another run's outputs (ref) -> None or the first difference; the three forms agree"""
    a, b = S["a"], S["b"]
    n = a.size
    j = np.arange(n) ^ 1
    j = np.where(j < n, j, np.arange(n))
    if ref is not None:
        w0, w1 = ref
    else:
        w = add_db_oracle(a, b, tab)
        w0, w1 = w, np.stack([w, w[j], w, w[j]], axis=1).ravel()
    bad = same_bits(out0, w0)
    if bad.size:
        return _bits_report("tl_add_db", _name_of(S, bad[0]), bad[0], dict(a=float(a[bad[0]]), b=float(b[bad[0]])), out0[bad[0]], w0[bad[0]]) + " (%d differ)" % bad.size
    bad = same_bits(out1, w1)
    if bad.size:
        i, k = divmod(int(bad[0]), 4)
        p = int(j[i]) if k & 1 else i
        return _bits_report(("tl_add_db2", "tl_add_db2_k")[k >> 1], _name_of(S, p) + (" (second pair)" if k & 1 else ""), p, dict(a=float(a[p]), b=float(b[p])), out1[bad[0]], w1[bad[0]]) + " (%d differ)" % bad.size
    o = out1.reshape(n, 4)
    if same_bits(o[:, 0], out0).size or same_bits(o[:, 2], out0).size:
        return "the three dB-sum forms disagree with one another"
    return None


def _name_of(S, i):
    for k, s in S["named"].items():
        if s.start <= i < s.stop:
            return "'%s'" % k
    return "?"


# ---- 2. masking terms
MASK_LEVELS = (TL_DBMIN, -100.0, -0.0625, 0.0, 15.0, 40.0, 96.3, 110.0)
MASK_X0 = (TL_DBMIN, -60.3, 0.0, 35.7, 96.3)


def mask_set():
    """-> dict(x, mb, aux [n, 4] = (line bark, x0, tonal, live), named)"""
    if "mask" in _args:
        return _args["mask"]
    _, _, barks = _emu_tables()
    pairs = []
    for key, t in barks.items():                                           # EVERY ordered pair (masker bark, line bark) of every table
        m, l = np.meshgrid(t, t, indexing="ij")
        pairs.append(np.stack([m.ravel(), l.ravel()], axis=1))
    pairs = np.unique(np.concatenate(pairs).view(U64), axis=0).view(np.float64)       # (tables share rows: each distinct pair once)
    npairs = pairs.shape[0]
    assert npairs > 100000
    X, MB, AUX, named = [], [], [], {}

    def add(name, x, mb, lb, x0, tonal, live):
        x, mb, lb, x0, tonal, live = (np.ravel(v).astype(np.float64) for v in np.broadcast_arrays(x, mb, lb, x0, tonal, live))
        s = sum(len(v) for v in X)
        X.append(x); MB.append(mb); AUX.append(np.stack([lb, x0, tonal, live], axis=1))
        named[name] = slice(s, s + x.size)

    lv = np.array(MASK_LEVELS)
    pi, li = np.meshgrid(np.arange(npairs), np.arange(8), indexing="ij")
    pi, li = pi.ravel(), li.ravel()
    add("every bark pair of the threshold tables x 8 levels", lv[li], pairs[pi, 0], pairs[pi, 1], np.array(MASK_X0)[(pi + li) % 5], (pi + li) & 1, ((pi >> 1) + li) & 1 ^ 1)
    # distances of exactly 0, +-1, -3, 8 and the doubles beside them: dz = line - masker, exact with one of the two at 0; and around 12 bark
    mbs, lbs = [], []
    for dz in (0.0, 1.0, -1.0, -3.0, 8.0):
        v = _near(abs(dz), 3)
        v = v[v >= 0]
        if dz >= 0:
            mbs.append(np.zeros(v.size)); lbs.append(v)
        if dz <= 0:
            mbs.append(v); lbs.append(np.zeros(v.size))
        w = _near(12.0 + dz, 3)
        mbs.append(np.full(w.size, 12.0)); lbs.append(w)
        mbs.append(w); lbs.append(np.full(w.size, 12.0 + 2 * dz) if 0 <= 12.0 + 2 * dz <= 32 else np.full(w.size, 12.0))
    mbs, lbs = np.concatenate(mbs), np.concatenate(lbs)
    g4 = np.array(np.meshgrid(np.arange(mbs.size), np.arange(8), [0, 1], [0, 1], indexing="ij")).reshape(4, -1)
    add("distances of exactly 0, +-1, -3, 8 and the doubles beside them", lv[g4[1]], mbs[g4[0]], lbs[g4[0]], np.array(MASK_X0)[(g4[0] + g4[1]) % 5], g4[2], g4[3])
    nmade = sum(len(v) for v in X)
    g = np.random.default_rng(42)
    n = NSTAGE_RANDOM
    add("random", g.uniform(-200.0, 120.0, n), g.uniform(0.0, 25.5, n), g.uniform(0.0, 25.5, n), g.uniform(-200.0, 120.0, n), g.integers(0, 2, n), g.integers(0, 2, n))
    S = dict(x=np.concatenate(X), mb=np.concatenate(MB), aux=np.ascontiguousarray(np.concatenate(AUX)), named=named, constructed=nmade, random=n)
    _args["mask"] = S
    return S


def mask_oracle(S, tab):
    """-> (record [n, 5], term [n], in reach [n], step [n]): av as written, the four-piece masking function, the reach test -3 <= dz < 8"""
    x, mb = S["x"], S["mb"]
    lb, x0, tonal = S["aux"][:, 0], S["aux"][:, 1], S["aux"][:, 2] != 0
    av = np.where(tonal, -1.525 - 0.275 * mb - 4.5 + x, -1.525 - 0.175 * mb - 0.5 + x)
    g, nn = 0.4 * x + 6, 17 - 0.15 * x
    dz = lb - mb
    vf = np.where(dz < -1, 17 * (dz + 1) - g, np.where(dz < 0, g * dz, np.where(dz < 1, -17 * dz, -(dz - 1) * nn - 17)))
    term = av + vf
    reach = (dz >= -3) & (dz < 8)
    step = np.where(reach, add_db_oracle(x0, term, tab), x0)
    return np.stack([mb, av, g, np.full(x.size, 17.0), nn], axis=1), term, reach, step


def mask_check(S, out0, out1, tab):
    rec, term, reach, step = mask_oracle(S, tab)
    arg = lambda i: dict(x=float(S["x"][i]), masker_bark=float(S["mb"][i]), line_bark=float(S["aux"][i, 0]), x0=float(S["aux"][i, 1]), tonal=int(S["aux"][i, 2]), live=int(S["aux"][i, 3]))
    o0, o1 = out0.reshape(-1, 8), out1.reshape(-1, 5)
    for k, name in enumerate(("bark", "av", "g", "c17", "n")):
        bad = same_bits(o1[:, k], rec[:, k])
        if bad.size:
            return _bits_report("tl_masker_consts." + name, _name_of(S, bad[0]), bad[0], arg(bad[0]), o1[bad[0], k], rec[bad[0], k]) + " (%d differ)" % bad.size
    live = S["aux"][:, 3] != 0
    for k, name in enumerate(("tl_mask_term", "tl_mask_term (other live)", "tl_mask_term_k", "tl_mask_term_k (other live)", "tl_mask_term_w", "tl_mask_term_w (other live)")):
        on = reach & (live if k % 2 == 0 else ~live)
        got = o0[:, k].view(U64)
        bad = np.flatnonzero(np.where(on, got != term.view(U64), (got >> U64(32)) != U64(FAR_HI)))
        if bad.size:
            i = bad[0]
            return _bits_report(name, _name_of(S, i) + (" in reach" if on[i] else " out of reach or not live: high word 0xC0F00000"), i, arg(i), o0[i, k], term[i]) + " (%d differ)" % bad.size
    bad = same_bits(o0[:, 6], step)
    if bad.size:
        return _bits_report("tl_mask_step", _name_of(S, bad[0]), bad[0], arg(bad[0]), o0[bad[0], 6], step[bad[0]]) + " (%d differ)" % bad.size
    return None


# ---- 3. masker spans
SPAN_NTONE = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127)
SPAN_NNOISE = (0, 1, 31, 32, 33, 63)


def _span_case(g, nt, nn, kind, slack, inv=None):
    """one case: the list (tones ascending, noise ascending; runs of equal barks for kind 'runs'), the slack behind it, 64 (blo, bhi)"""
    nm = nt + nn
    step = 0.25 if kind == "runs" else 0.001
    mk = lambda n: np.sort(np.round(g.uniform(0.0, 25.0, n) / step) * step)
    lst = np.concatenate([mk(nt), mk(nn)])
    if inv == "seam" and nt and nn:                                        # the seam alone: the first noise bark below the last tone's
        lst[:nt] = np.maximum(lst[:nt], 1.0)
        lst[nt] = 0.5 * lst[nt - 1]
        lst[nt:] = np.sort(lst[nt:])
    elif inv is not None:                                                  # an inversion at q: list[q] < list[q - 1]
        q = inv
        lst[q - 1], lst[q] = max(lst[q - 1], lst[q]) + 0.5, min(lst[q - 1], lst[q])
    full = np.empty(LIST)
    full[:nm] = lst
    lo, hi = (lst.min(), lst.max()) if nm else (5.0, 6.0)
    full[nm:] = -1e300 if slack == 0 else g.uniform(lo, hi, LIST - nm) if slack == 1 else np.round(g.uniform(lo, hi, LIST - nm) / 0.25) * 0.25
    b = np.empty((64, 2))
    c = g.uniform(0.0, 25.0, 64)
    b[:, 0], b[:, 1] = c - 8.0, c + 3.0                                    # the callers' spans
    pick = lambda n: lst[g.integers(0, nm, n)] if nm else g.uniform(0.0, 25.0, n)
    b[0:8, 0] = pick(8)                                                    # a bound equal to a list value
    b[8:16, 1] = pick(8)
    b[16:20, 0], b[16:20, 1] = pick(4), pick(4)                            # both (half of them empty: bhi <= blo)
    v = pick(4)
    b[20:24, 0] = b[20:24, 1] = v                                          # blo = bhi
    b[24] = (lo, hi); b[25] = (np.nextafter(lo, -1), hi); b[26] = (lo, np.nextafter(hi, -1)); b[27] = (hi, hi + 1)      # the first, the last
    b[28] = (-5.0, lo - 1e-9 if lo > 0 else -1.0); b[29] = (hi, 40.0); b[30] = (-10.0, 40.0); b[31] = (20.0, 3.0)       # below all, above all, everything, empty
    if nt:
        b[32] = (lst[nt - 1], 40.0); b[33] = (-1.0, lst[0]); b[34] = (np.nextafter(lst[nt - 1], -1), lst[nt - 1])
    if nn:
        b[35] = (lst[nm - 1], 40.0); b[36] = (-1.0, lst[nt]); b[37] = (np.nextafter(lst[nm - 1], -1), lst[nm - 1])
    return full, b


def spans_set():
    """-> dict(list [n, 192], bounds [n, 64, 2], counts [n, 2], named)"""
    if "spans" in _args:
        return _args["spans"]
    g = np.random.default_rng(43)
    Ls, Bs, Cs, names = [], [], [], []

    def add(name, nt, nn, *a, **k):
        full, b = _span_case(g, nt, nn, *a, **k)
        Ls.append(full); Bs.append(b); Cs.append((nt, nn)); names.append(name)

    for nt in SPAN_NTONE:
        for nn in SPAN_NNOISE:
            if nt + nn > MASKER_MAX:
                continue
            for kind in ("plain", "runs"):
                for slack in (0, 1, 2):
                    add("sorted %s, slack %d" % (kind, slack), nt, nn, kind, slack)
            nm = nt + nn
            for q in sorted({1, nm - 1, 64, 65} - {nt}):                   # unsorted: at q = 1, the last element, the lane wrap -- never AT the seam here
                if 1 <= q < nm:
                    add("inversion at q = %d" % q, nt, nn, "plain", q & 1, inv=q)
            if nt and nn:
                add("inversion at the seam alone", nt, nn, "plain", 0, inv="seam")
                add("inversion at the seam alone", nt, nn, "runs", 1, inv="seam")
    add("gate: 128 tones", 128, 0, "plain", 0)
    add("gate: 64 noise components", 64, 64, "plain", 1)
    add("gate: 64 noise components", 0, 64, "runs", 0)
    nmade = len(Ls)
    for _ in range(2048):
        nt = int(g.integers(0, 128))
        nn = int(g.integers(0, min(63, MASKER_MAX - nt) + 1))
        nm = nt + nn
        inv = int(g.integers(1, nm)) if nm > 1 and g.integers(0, 5) == 0 else None
        add("random", nt, nn, ("plain", "runs")[int(g.integers(0, 2))], int(g.integers(0, 3)), inv=inv)
    S = dict(list=np.array(Ls), bounds=np.array(Bs), counts=np.array(Cs, dtype=I32), names=names, constructed=nmade, random=2048)
    _args["spans"] = S
    return S


def spans_oracle(S):
    """a plain look at every masker: the first and last index with blo < bark <= bhi among the tones and among the noise components
    (empty: nm, -1); sorted: all(mb[q] >= mb[q - 1] for q != ntone)"""
    lst, b, cnt = S["list"][:, :MASKER_MAX], S["bounds"], S["counts"].astype(np.int64)
    n = lst.shape[0]
    q = np.arange(MASKER_MAX)[None, None, :]
    nt, nm = cnt[:, 0][:, None, None], cnt.sum(axis=1)[:, None, None]
    hit = (lst[:, None, :] > b[:, :, 0:1]) & (lst[:, None, :] <= b[:, :, 1:2]) & (q < nm)
    out = np.empty((n, 64, 4), dtype=np.int64)
    for k, part in enumerate((hit & (q < nt), hit & (q >= nt))):
        some = part.any(axis=2)
        out[:, :, 2 * k] = np.where(some, part.argmax(axis=2), nm[:, :, 0])
        out[:, :, 2 * k + 1] = np.where(some, MASKER_MAX - 1 - part[:, :, ::-1].argmax(axis=2), -1)
    qq = np.arange(1, MASKER_MAX)[None, :]
    down = (lst[:, 1:] < lst[:, :-1]) & (qq < nm[:, :, 0]) & (qq != nt[:, :, 0])
    srt = ~down.any(axis=1)
    return out, srt


def spans_check(S, out0, out1):
    want, srt = spans_oracle(S)
    o = out0.reshape(-1, 64, 8).astype(np.int64)
    flags = out1.reshape(-1, 2)
    cnt = S["counts"]
    bad = np.flatnonzero(flags[:, 0] != srt)
    if bad.size:
        return "tl_maskers_sorted, case %d (%s, ntone %d, nnoise %d): %d, want %d (%d differ)" % (bad[0], S["names"][bad[0]], cnt[bad[0], 0], cnt[bad[0], 1], flags[bad[0], 0], srt[bad[0]], bad.size)
    gate = srt & (cnt[:, 0] < 128) & (cnt[:, 1] < 64)
    bad = np.flatnonzero(flags[:, 1] != gate)
    if bad.size:
        return "the callers' gate, case %d (%s): %d, want %d" % (bad[0], S["names"][bad[0]], flags[bad[0], 1], gate[bad[0]])
    for name, got, ref in (("tl_mask_spans", o[:, :, :4], want), ("tl_mask_spans_sorted", o[:, :, 4:], np.where(gate[:, None, None], want, -2))):
        bad = np.argwhere((got != ref).any(axis=2))
        if bad.size:
            c, l = bad[0]
            return "%s, case %d (%s, ntone %d, nnoise %d), lane %d, blo=%s bhi=%s: %s, want %s (%d lanes differ)" % (
                name, c, S["names"][c], cnt[c, 0], cnt[c, 1], l, float(S["bounds"][c, l, 0]).hex(), float(S["bounds"][c, l, 1]).hex(), got[c, l].tolist(), ref[c, l].tolist(), bad.shape[0])
    return None


# ---- 4. tl_min_rows
MIN_ROWS_N = (1, 2, 3, 4, 5, 6, 7, 8, 9, 27)


def min_rows_set():
    """-> dict(col [n, 136], m [n, 64], rows [n, 64, 3] = (j0, n, take_first)): per case one column and 64 lanes over (n, take_first, m below /
    among / above the rows)"""
    if "min_rows" in _args:
        return _args["min_rows"]
    g = np.random.default_rng(44)
    cols = []
    pz, nz = 0.0, -0.0
    for rep in range(6):
        base = g.normal(20.0, 30.0, ROWS)
        cols += [base, np.round(base / 20.0) * 20.0,                                        # few distinct values: duplicates
                 np.tile([pz, nz], ROWS // 2), np.tile([nz, pz], ROWS // 2),                # +0.0 / -0.0 neighbours, both orders
                 np.where(g.integers(0, 3, ROWS) == 0, np.tile([pz, nz], ROWS // 2), np.abs(base) + 1.0),      # zeros are the minima, among positive rows
                 np.where(g.integers(0, 3, ROWS) == 0, np.tile([nz, pz], ROWS // 2), np.abs(base) + 1.0),
                 np.where(g.integers(0, 2, ROWS) == 0, np.tile([nz, nz, pz, pz], ROWS // 4), np.tile([pz, nz], ROWS // 2)),
                 np.sort(base), np.sort(base)[::-1], np.full(ROWS, 7.5)]
    nmade = len(cols)
    cols += [g.normal(20.0, 30.0, ROWS) for _ in range(192)] + [np.round(g.normal(0.0, 1.0, ROWS)) * g.choice([0.0, -0.0, 1.0], ROWS) for _ in range(64)]
    col = np.array(cols)
    n = col.shape[0]
    rows = np.empty((n, 64, 3), dtype=I32)
    m = np.empty((n, 64))
    for c in range(n):
        for l in range(64):
            cnt = MIN_ROWS_N[l % 10] if l < 60 else (27, 9, 4, 1)[l - 60]
            tf = (l // 10) & 1
            j0 = (0, ROWS - cnt)[l & 1] if (c % 3 == 0 and l < 60) else int(g.integers(0, ROWS - cnt + 1))
            seg = col[c, j0:j0 + cnt]
            kind = (l // 20) % 3 if l < 60 else l - 60
            m[c, l] = (seg.min() - 10.0, seg[int(g.integers(0, cnt))], 999999.9, 0.0)[kind]
            rows[c, l] = (j0, cnt, tf)
    S = dict(col=col, m=m, rows=rows, constructed=nmade * 64, random=(n - nmade) * 64)
    _args["min_rows"] = S
    return S


def min_rows_oracle(S):
    """the reference's running minimum: m = row j0 first (take_first) or the given m, then `if m > v: m = v` row by row -- the first zero met stays"""
    col, rows = S["col"], S["rows"].astype(np.int64)
    m = S["m"].copy()
    c = np.arange(col.shape[0])[:, None]
    for r in range(27):
        on = r < rows[:, :, 1]
        v = col[c, np.minimum(rows[:, :, 0] + r, ROWS - 1)]
        take = on & ((m > v) | ((r == 0) & (rows[:, :, 2] != 0)))
        m = np.where(take, v, m)
    return m


def min_rows_check(S, out0):
    want = min_rows_oracle(S)
    bad = np.argwhere(out0.reshape(want.shape).view(U64) != want.view(U64))
    if bad.size:
        c, l = bad[0]
        j0, cnt, tf = S["rows"][c, l]
        return "tl_min_rows, case %d lane %d: rows [%d, %d) = %s, m = %s, take_first = %d -> %s, want %s (%d differ)" % (
            c, l, j0, j0 + cnt, [float(v).hex() for v in S["col"][c, j0:j0 + cnt]], float(S["m"][c, l]).hex(), tf, float(out0.reshape(want.shape)[c, l]).hex(), float(want[c, l]).hex(), bad.shape[0])
    return None


# ---- 5. tl_mnr_key
def mnr_key_set():
    if "mnr_key" in _args:
        return _args["mnr_key"]
    g = np.random.default_rng(45)
    lim = 999999.0
    made = np.concatenate([_pm(np.concatenate([[0.0, MINSUB, MINN, 1e-300, 1e-20, 0.1, 1.0, 96.3, 999998.0, 1e6, 1e7, 1e300, MAXN], ONES, POW2_ALL[::16]])),
                           _near(lim, 8), _near(-lim, 2), np.arange(-120, 121) * 0.5, _near(999999.9, 1)])
    rnd = np.concatenate([g.normal(0.0, 40.0, NSTAGE_RANDOM // 2), g.choice([-1.0, 1.0], NSTAGE_RANDOM // 2) * np.ldexp(g.uniform(1.0, 2.0, NSTAGE_RANDOM // 2), g.integers(-1074, 1024, NSTAGE_RANDOM // 2).astype(np.int32))])
    S = dict(x=np.concatenate([made, rnd]), constructed=made.size, random=rnd.size)
    _args["mnr_key"] = S
    return S


def mnr_key_oracle(x):
    """Python integers on the bits: below 999999.0 the bits of x (a zero of either sign as +0) with the sign bit set for x >= 0, inverted for x < 0; else ~0"""
    out = []
    for u, v in zip(_d2u(x).tolist(), x.tolist()):
        if not (999999.0 > v):
            out.append((1 << 64) - 1)
            continue
        if v == 0.0:
            u = 0
        out.append(((1 << 64) - 1 - u) if u >> 63 else (u | (1 << 63)))
    return out


def mnr_key_check(S, out0):
    x = S["x"]
    want = mnr_key_oracle(x)
    got = out0.tolist()
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            return "tl_mnr_key: argument %d = %s -> %#x, want %#x" % (i, float(x[i]).hex(), a, b)
    # what the allocation relies on: ascending doubles give strictly ascending keys; +-0.0 one key; from 999999.0 on exactly ~0
    xs = np.unique(x[x < 999999.0])                                        # (sorted; -0.0 and 0.0 are one value here)
    ks = np.array([got[i] for i in np.unique(x, return_index=True)[1]], dtype=U64)[:xs.size]
    if not (ks[1:] > ks[:-1]).all():
        i = int(np.flatnonzero(~(ks[1:] > ks[:-1]))[0])
        return "tl_mnr_key: keys of %s and %s do not ascend" % (float(xs[i]).hex(), float(xs[i + 1]).hex())
    k0 = {got[i] for i in np.flatnonzero(x == 0.0)}
    if len(k0) != 1:
        return "tl_mnr_key: +0.0 and -0.0 have different keys"
    if not all(got[i] == (1 << 64) - 1 for i in np.flatnonzero(x >= 999999.0)) or any(got[i] == (1 << 64) - 1 for i in np.flatnonzero(x < 999999.0)):
        return "tl_mnr_key: ~0 is not exactly the keys from 999999.0 on"
    return None


# ---- 6. scalefactor index and count
def scalefactors():
    return _emu_tables()[1]


def sf_index_set(sf):
    """the set of tests/test_emu_parity.py test_scalefactor_index: every table entry and its neighbours, powers of two and their neighbours, random
    magnitudes over the whole range, zero and denormals -- below 2.0"""
    rng = np.random.default_rng(11)
    p2 = 2.0 ** np.arange(-80, 1)
    vals = np.concatenate([sf, np.nextafter(sf, 0), np.nextafter(sf, 4), p2, np.nextafter(p2, 0), np.nextafter(p2, 4),
                           10.0 ** rng.uniform(-25, 0.3, 400000), rng.uniform(0, 2, 400000), [0.0, 5e-324, 1e-310, 1e-300, 1.999999]])
    return np.ascontiguousarray(vals[vals < 2.0])


def sf_index_check(vals, sf, out0, out1):
    """both searches == (number of table entries >= the argument) - 1, 0 when there is none; tl_sfs_count(i) = 3, 2, 1, 2 for scfsi i & 3"""
    asc = sf[::-1]
    assert (np.diff(asc) > 0).all()
    cnt = 64 - np.searchsorted(asc, vals, side="left")
    want = np.maximum(cnt - 1, 0)
    o = out0.reshape(-1, 2)
    for k, name in enumerate(("tl_sf_index", "tl_sf_index_ref")):
        bad = np.flatnonzero(o[:, k] != want)
        if bad.size:
            return "%s: argument %d = %s -> %d, want %d (%d differ)" % (name, bad[0], float(vals[bad[0]]).hex(), o[bad[0], k], want[bad[0]], bad.size)
    bad = np.flatnonzero(out1 != np.array([3, 2, 1, 2])[np.arange(vals.size) & 3])
    if bad.size:
        return "tl_sfs_count(%d) = %d" % (bad[0], out1[bad[0]])
    return None


# ---- 7. tl_div_by
def hardest(d):
    """Dividends whose quotient by d lies within ~2^-106 (relative) of a rounding midpoint: S * 2^53 = (2M+1) * D + t
    for small t, solved for the odd 2M+1 modulo a power of two (D = integer significand of d)."""
    import math
    m, e = math.frexp(d)
    D = int(m * (1 << 53))
    z = (D & -D).bit_length() - 1
    Dp, mod = D >> z, 1 << (53 - z)
    inv = pow(Dp, -1, mod)
    out = []
    for tp in range(-15, 16, 2):
        r = (-tp * inv) % mod
        for k in range(0, 1 << z if z < 6 else 64):
            o = r + k * mod
            if not (o & 1):
                continue
            o |= 1 << 53                                        # 2M+1 in [2^53, 2^54)
            num = o * D + (tp << z)
            if num % (1 << 53):
                continue
            S = num >> 53
            while S >= (1 << 53) and not (S & 1):
                S >>= 1
            if (1 << 52) <= S < (1 << 53):
                out.append(math.ldexp(float(S), -52))
    return out


def div_by_sets(sf, n):
    """the sets of tests/test_emu_parity.py test_quantiser_division, divisor by divisor -> (d, dividends, number of hardest() dividends): n random
    dividends over the subband-sample range, n exact multiples, n next to a representable quotient, 3 n next to a rounding midpoint, and
    every hardest() dividend of both signs.  Divisors: the scalefactors; the critical-band widths 1..200 (psy 1 noise weights)."""
    rng = np.random.default_rng(7)
    for d in np.concatenate([sf, np.arange(1.0, 201.0)]):
        s_rand = rng.uniform(-2.5, 2.5, n) * 10.0 ** rng.uniform(-12, 0, n)
        q = rng.uniform(0.5, 4.0, n) * rng.choice([-1.0, 1.0], n)
        near_rep = np.nextafter(q * d, rng.choice([-np.inf, np.inf], n))      # quotient within an ulp of q
        half = (np.nextafter(np.abs(q), np.inf) - np.abs(q)) / 2
        mid = (np.abs(q).astype(np.longdouble) + half.astype(np.longdouble)) * np.sign(q).astype(np.longdouble)
        near_mid = (mid * np.longdouble(d)).astype(np.float64)              # quotient within an ulp-fraction of a midpoint
        hard = np.array(hardest(float(d)), dtype=np.float64)
        s_all = np.ascontiguousarray(np.concatenate([s_rand, q * d, near_rep, near_mid, np.nextafter(near_mid, np.inf),
                                                     np.nextafter(near_mid, -np.inf), hard, -hard]))
        yield float(d), s_all, len(hard)


def div_by_set():
    """the probe's set: each randomly drawn class (uniform, exact multiple, next to a representable quotient, next to a midpoint and its two
    neighbours) thinned to 2^14 draws per divisor, every hardest() dividend of both signs kept, and a zero dividend of either sign per divisor"""
    if "div_by" in _args:
        return _args["div_by"]
    Ss, Ds, Cl, nhard, n = [], [], [], 0, 1 << 14
    for d, s, nh in div_by_sets(scalefactors(), n):
        Ss.append(s); Ds.append(np.full(s.size, d)); nhard += 2 * nh
        Cl.append(np.concatenate([np.repeat(np.arange(6, dtype=np.int8), n), np.full(2 * nh, 6, dtype=np.int8)]))
        Ss.append(np.array([0.0, -0.0])); Ds.append(np.full(2, d)); Cl.append(np.full(2, 7, dtype=np.int8))
    s, d = np.concatenate(Ss), np.concatenate(Ds)
    S = dict(cls=np.concatenate(Cl), s=s, d=d, constructed=s.size - 6 * 264 * (1 << 14), random=6 * 264 * (1 << 14), hardest=nhard)
    _args["div_by"] = S
    return S


def div_by_check(S, out0, out1):
    """numpy's s / d; where the dividend is a zero, compared after + 0.0 (the header documents the sign)"""
    s, d = S["s"], S["d"]
    want = s / d
    z = s == 0.0
    for name, got in (("tl_div_by (reciprocal made in the kernel)", out0), ("tl_div_by (reciprocal made on the host)", out1)):
        bad = same_bits(np.where(z, got + 0.0, got), np.where(z, want + 0.0, want))
        if bad.size:
            what = ("'random'", "'exact multiple'", "'next to a representable quotient'", "'next to a midpoint'", "'above one next to a midpoint'", "'below one next to a midpoint'", "'hardest()'", "'zero dividend'")
            cl = np.bincount(S["cls"][bad], minlength=8)
            if cl[6]:                                                      # a constructed dividend first
                bad = bad[S["cls"][bad] == 6]
            return _bits_report(name, what[S["cls"][bad[0]]] + " " + str(cl.tolist()), bad[0], dict(s=float(s[bad[0]]), d=float(d[bad[0]])), got[bad[0]], want[bad[0]]) + " (%d differ)" % bad.size
    return None


# ---- 8. bit writer and CRC
def bits_set(wide):
    """-> dict(val [n, 64, 6] u64, len [n, 64, 6] i32, par [n, 2] = (start, wide)).  tl_put_bits: lengths 0..32, zeros included; tl_put_bits48: 1..48
    (0 = no field: its callers skip one)"""
    key = "bits%d" % wide
    if key in _args:
        return _args[key]
    g = np.random.default_rng(46 + wide)
    top = 48 if wide else 32
    lens, vals, starts, names = [], [], [], []

    def add(name, start, ln, ones=False):
        ln = np.asarray(ln, dtype=np.int64).reshape(64, FIELDS)
        assert start + ln.sum() <= FRAME_BITS and ln.min() >= 0 and ln.max() <= top
        full = (np.ones((64, FIELDS), dtype=U64) << ln.astype(U64)) - U64(1)
        v = full if ones else g.integers(0, 1 << 63, (64, FIELDS), dtype=U64) & full
        lens.append(ln.astype(I32)); vals.append(v); starts.append(start); names.append(name)

    for start in range(64):                                                # every start offset
        add("start offset, random lengths", start, g.integers(0 if not wide else 1, top + 1, (64, FIELDS)))
        add("start offset, all-ones values", start, g.integers(1, top + 1, (64, FIELDS)), ones=True)
    for start in (0, 1, 31, 32, 33, 63):
        ln = g.integers(1, top + 1, (64, FIELDS))
        pos = start
        for l in range(64):                                                # every lane's third and last field end exactly on a word boundary
            for f in range(FIELDS):
                if f in (2, 5):
                    r = (-pos) % 32
                    ln[l, f] = r if r else 32
                pos += ln[l, f]
        add("fields ending on a word boundary", start, ln, ones=start & 1)
        add("short fields: neighbouring lanes share a word", start, g.integers(0 if not wide else 1, 6, (64, FIELDS)), ones=start == 63)
        add("one-bit fields", start, np.ones((64, FIELDS)), ones=True)
        if wide:
            ln = np.zeros((64, FIELDS), dtype=np.int64)
            ln[:, :4] = 48                                                 # a 48-bit field at offset o > 16 spans three words: every offset occurs (48 l + start mod 32)
            add("48-bit fields spanning three words", start, ln, ones=True)
            ln = g.integers(33, 49, (64, FIELDS))
            ln[:, 4:] = 0
            add("fields of 33..48 bits", start, ln)
        else:
            add("32-bit fields", start, np.full((64, FIELDS), 32), ones=True)
            ln = g.integers(0, 33, (64, FIELDS))
            ln[g.integers(0, 2, (64, FIELDS)) == 0] = 0
            add("many empty fields", start, ln)
    nmade = len(lens)
    for _ in range(256):
        add("random", int(g.integers(0, 64)), g.integers(0 if not wide else 1, top + 1, (64, FIELDS)), ones=bool(g.integers(0, 4) == 0))
    S = dict(val=np.array(vals), len=np.array(lens), par=np.array([(s, wide) for s in starts], dtype=I32), names=names, constructed=nmade, random=256)
    _args[key] = S
    return S


def _crc_lanes(val, ln, poly, top, init):
    """a bitwise CRC (crc.c:43-56 / :99-113) of each lane's fields, MSB first, all lanes side by side"""
    crc = np.full(val.shape[:2], init, dtype=np.int64)
    mask = 2 * top - 1
    for f in range(FIELDS):
        v, nb = val[:, :, f], ln[:, :, f].astype(np.int64)
        for k in range(int(nb.max())):
            on = k < nb
            bit = ((v >> np.maximum(nb - 1 - k, 0).astype(U64)) & U64(1)).astype(np.int64)
            carry = (crc & top) != 0
            new = ((crc << 1) & mask) ^ np.where(carry != (bit != 0), poly, 0)
            crc = np.where(on, new, crc)
    return crc


def bits_oracle(S):
    """the frame as one Python integer: the fields MSB first at running offsets from `start`; its words, their byte swaps; the CRCs"""
    val, ln = S["val"], S["len"]
    n = val.shape[0]
    words = np.empty((n, FRAME_WORDS), dtype=np.uint32)
    nbits = 32 * FRAME_WORDS
    for c in range(n):
        big, pos = 0, int(S["par"][c, 0])
        for v, nb in zip(val[c].ravel().tolist(), ln[c].ravel().tolist()):
            big |= v << (nbits - pos - nb)
            pos += nb
        words[c] = np.frombuffer(big.to_bytes(4 * FRAME_WORDS, "big"), dtype=">u4")
    swapped = words.byteswap()
    crc = np.stack([_crc_lanes(val, ln, 0x8005, 0x8000, 0xffff), _crc_lanes(val, ln, 0x1d, 0x80, 0)], axis=2)
    return words, swapped, crc


def bits_check(S, out0, out1):
    words, swapped, crc = bits_oracle(S)
    o = out0.reshape(-1, 3, FRAME_WORDS)
    name = "tl_put_bits48" if S["par"][0, 1] else "tl_put_bits"
    for k, (what, ref) in enumerate(((name + ": frame word", words), ("tl_get_bit: frame word read bit by bit", words), ("tl_bswap of frame word", swapped))):
        bad = np.argwhere(o[:, k] != ref)
        if bad.size:
            c, w = bad[0]
            return "%s %d of case %d (%s, start %d): %#010x, want %#010x (%d words differ)" % (what, w, c, S["names"][c], S["par"][c, 0], o[c, k, w], ref[c, w], bad.shape[0])
    bad = np.argwhere(out1.reshape(-1, 64, 2).astype(np.int64) != crc)
    if bad.size:
        c, l, k = bad[0]
        return "tl_crc_upd (%s) of case %d lane %d: fields %s lengths %s -> %#x, want %#x" % (("CRC-16", "ScF-CRC")[k], c, l, [hex(int(v)) for v in S["val"][c, l]], S["len"][c, l].tolist(),
                                                                                             out1.reshape(-1, 64, 2)[c, l, k], crc[c, l, k])
    return None


# ---- 9. the bit allocation (csrc/mp2_alloc.h: tl_allocate, tl_allocate_pair), one layer above the helpers
# The oracle is the reference's own loop (a_bit_allocation_new with maxmnr_new, encode_new.c:1061-1187) restated from its definition, one
# event at a time: the smallest MNR = SNR - SMR in double, first in (channel, subband) order by the scan's strict `>` against the 999999.0
# sentinel; the step's price (samples; at a cell's first step the scfsi code and the scalefactors, of both channels above jsbound); a step
# that does not fit closes its cell for good (used = 2), so does the line's last allocation; above jsbound the partner channel copies the
# winner's allocation and state.  No key, no round, nothing of csrc/ but the Layer II tables of mp2_tables.inc as they stand there.  All
# cases advance in lockstep (one event of every unfinished case per pass) -- numpy over the cases, not over the algorithm.  tests/
# test_alloc_oracle_golden.py pins it to the reference's bit_alloc taps.
ALLOC_MAX_ADB = 8 * 1728                                                   # 8 * TL_MAX_FRAME_BYTES
ALLOC_SMALL = 999999.0
SFS_PER_SCFSI = np.array([3, 2, 1, 2])
ALLOC_COVER = 32                                                           # cases of each form of call that must meet each coverage condition


def _alloc_tables():
    if "alloc_tables" not in _built:
        L = emu()
        buf = np.zeros(18 * 3 + 9 + 144 + 160 + 5, dtype=I32)
        L.probe_alloc_tables.argtypes, L.probe_alloc_tables.restype = [C.c_void_p], None
        L.probe_alloc_tables(_ptr(buf))
        o = np.cumsum([0, 18, 18, 18, 9, 144, 160, 5])
        snr_e2, bits, group, nbal, step, line, sbl = (buf[o[i]:o[i + 1]].astype(np.int64) for i in range(7))
        _built["alloc_tables"] = dict(snr=snr_e2 / 100.0, bits12=12 * group * bits, nbal=nbal, step=step.reshape(9, 16), line=line.reshape(5, 32), sblimit=sbl)
    return _built["alloc_tables"]


def _alloc_geometry(tab, nch, jsb):
    """per case: line and nbal per subband (0 above sblimit), the last allocation of each line, live cells [n, 2, 32], joint subbands, bbal"""
    T = _alloc_tables()
    sb = np.arange(32)
    sbl = T["sblimit"][tab]
    insb = sb[None, :] < sbl[:, None]
    line = np.where(insb, T["line"][tab], 0)
    nbal = np.where(insb, T["nbal"][line], 0)
    live = insb[:, None, :] & (np.arange(2)[None, :, None] < nch[:, None, None])
    joint = insb & (nch[:, None] == 2) & (sb[None, :] >= jsb[:, None])
    bbal = (nbal * np.where(sb[None, :] < jsb[:, None], nch[:, None], 1)).sum(axis=1)
    return line, (1 << nbal) - 1, live, joint, bbal


def alloc_greedy(tab, nch, jsb, adb, smr, scfsi):
    """n cases.  tab, nch, jsb, adb: int [n]; smr double [n, 2, 32], scfsi [n, 2, 32] (cells that are not live are not looked at)
    -> dict(ba [n, 2, 32], left [n], ad [n], and the trace: per event e of case i  cell [n, E] (32 ch + sb; -1 behind the case's last event),
    price [n, E], ok [n, E] (admitted / refused), tied [n, E] (another cell, not the joint partner, had the same MNR), xlevel [n, E] (... at
    another allocation level), ch1 [n, E] (a joint pair's event won by channel 1))"""
    T = _alloc_tables()
    tab, nch, jsb, adb = (np.asarray(v, dtype=np.int64) for v in (tab, nch, jsb, adb))
    smr = np.asarray(smr, dtype=np.float64)
    n = tab.size
    rows = np.arange(n)
    line, maxa, live, joint, bbal = _alloc_geometry(tab, nch, jsb)
    ad = adb - (bbal + 16 + 32)
    snr_of = lambda ln, b: T["snr"][T["step"][ln, b]]
    b12_of = lambda ln, b: T["bits12"][T["step"][ln, b]]
    mnr = T["snr"][0] - smr
    used = np.where(live, 0, 2)
    ba = np.zeros((n, 2, 32), dtype=np.int64)
    spent = np.zeros(n, dtype=np.int64)                                    # bspl + bscf + bsel
    sfs = 6 * SFS_PER_SCFSI[np.asarray(scfsi, dtype=np.int64)]
    cand = np.where(used != 2, mnr, np.inf)                                # what maxmnr_new may still pick
    steps = []
    while True:
        flat = cand.reshape(n, 64)
        idx = flat.argmin(axis=1)                                          # the first of equal minima in (ch, sb) order: the scan's strict `>`
        val = flat[rows, idx]
        r = np.flatnonzero(val < ALLOC_SMALL)
        if not r.size:
            break
        ch, s = idx[r] // 32, idx[r] % 32
        oth = 1 - ch
        ln, cur = line[r, s], ba[r, ch, s]
        first = used[r, ch, s] == 0
        jn = joint[r, s]
        inc = b12_of(ln, cur + 1) - np.where(first, 0, b12_of(ln, cur))
        seli = np.where(first, 2 + 2 * jn, 0)
        scale = np.where(first, sfs[r, ch, s] + np.where(jn, sfs[r, oth, s], 0), 0)
        price = inc + seli + scale
        ok = ad[r] >= spent[r] + price
        eq = cand[r] == val[r][:, None, None]
        ncell = np.where(joint[r], eq[:, 0] | eq[:, 1], eq[:, 0].astype(np.int64) + eq[:, 1]).sum(axis=1)
        lv_hi, lv_lo = np.where(eq, ba[r], -1).max(axis=(1, 2)), np.where(eq, ba[r], 99).min(axis=(1, 2))
        steps.append((r, idx[r], price, ok, ncell > 1, (ncell > 1) & (lv_hi != lv_lo), jn & (ch == 1)))
        nb = cur + ok
        ba[r, ch, s] = nb
        spent[r] += np.where(ok, price, 0)
        u = np.where(ok & (nb < maxa[r, s]), 1, 2)
        used[r, ch, s] = u
        mnr[r, ch, s] = np.where(ok, snr_of(ln, nb) - smr[r, ch, s], mnr[r, ch, s])
        cand[r, ch, s] = np.where(u != 2, mnr[r, ch, s], np.inf)
        j = np.flatnonzero(jn)                                             # above jsbound the allocation applies to both channels
        rj, sj, oj = r[j], s[j], oth[j]
        ba[rj, oj, sj] = nb[j]
        used[rj, oj, sj] = u[j]
        mnr[rj, oj, sj] = snr_of(ln[j], nb[j]) - smr[rj, oj, sj]
        cand[rj, oj, sj] = np.where(u[j] != 2, mnr[rj, oj, sj], np.inf)
    E = len(steps)
    out = dict(ba=np.where(live, ba, 0), left=ad - spent, ad=ad, cell=np.full((n, E), -1, dtype=np.int16), price=np.zeros((n, E), dtype=I32),
               ok=np.zeros((n, E), dtype=bool), tied=np.zeros((n, E), dtype=bool), xlevel=np.zeros((n, E), dtype=bool), ch1=np.zeros((n, E), dtype=bool),
               saturated=(np.where(live, ba, maxa[:, None, :]) == maxa[:, None, :]).all(axis=(1, 2)))
    for e, (r, cell, price, ok, tied, xl, c1) in enumerate(steps):
        out["cell"][r, e], out["price"][r, e], out["ok"][r, e], out["tied"][r, e], out["xlevel"][r, e], out["ch1"][r, e] = cell, price, ok, tied, xl, c1
    return out


def alloc_facts(R):
    """what the coverage conditions ask of a trace, per case"""
    ok, there = R["ok"], R["cell"] >= 0
    E = ok.shape[1]
    pos = np.arange(E)[None, :]
    first_no = np.where(there & ~ok, pos, E).min(axis=1) if E else np.zeros(ok.shape[0], dtype=np.int64)
    last_ok = np.where(ok, pos, -1).max(axis=1) if E else np.full(ok.shape[0], -1)
    return dict(tied=R["tied"].any(axis=1), xlevel=R["xlevel"].any(axis=1), refused_then_admitted=first_no < last_ok, left_zero=R["left"] == 0,
                nothing=~ok.any(axis=1), saturated=R["saturated"], ch1=(R["ch1"] & ok).any(axis=1), events=there.sum(axis=1), free=first_no)


ALLOC_SMR_KINDS = ("random", "all cells equal", "channels identical", "a short list of integers", "cells at different levels tie", "extremes -200 / 0 / 96",
                   "upper channel first")


def _alloc_smr(g, kind, tab, T):
    """-> smr [2, 32], scfsi [2, 32]: every cell filled, live or not (what is not live must not matter)"""
    smr = g.uniform(-30.0, 60.0, (2, 32))
    sel = g.integers(0, 4, (2, 32))
    if kind == "all cells equal":
        smr[:] = g.choice([-7.0, 0.0, 3.5, 20.0, 41.0])
        if g.integers(0, 2):
            sel[:] = g.integers(0, 4)
    elif kind == "channels identical":
        smr[1] = smr[0]
        if g.integers(0, 2):
            sel[1] = sel[0]
    elif kind == "a short list of integers":
        smr = g.choice([-3.0, 0.0, 2.0, 5.0, 9.0, 12.0, 20.0], (2, 32))
    elif kind == "cells at different levels tie":
        # SMRs that put cells at DIFFERENT allocation levels on the same MNR m: smr = snr(line, level) - m, kept only where snr - smr gives m
        # back on the bits (m a multiple of 1/64: the difference is then usually exact); two values of m per case
        line = np.where(T["line"][tab] == 255, 0, T["line"][tab])
        top = (1 << T["nbal"][line]) - 1
        for m in g.integers(-20 * 64, 30 * 64, 2) / 64.0:
            lvl = g.integers(0, np.broadcast_to(top, (2, 32)))
            snr = T["snr"][T["step"][np.broadcast_to(line, (2, 32)), lvl]]
            v = snr - m
            take = (snr - v == m) & (g.random((2, 32)) < 0.45)
            smr = np.where(take, v, smr)
    elif kind == "extremes -200 / 0 / 96":
        smr = g.choice([-200.0, 0.0, 96.0], (2, 32))
    elif kind == "upper channel first":                                   # channel 1 has the larger SMR, so the smaller MNR: a joint pair acts on the partner's key
        smr[1] = smr[0] + g.uniform(0.5, 25.0, 32)
    return smr, sel


ALLOC_BUDGETS = ("bbal + 48: nothing fits", "a few bits: nothing fits", "exactly the first event", "exactly the events up to k", "one bit short of the events up to k",
                 "exactly the events up to k'", "one bit short of the events up to k'", "the largest frame", "random")


def _alloc_budget(g, kind, bbal, cum, ncell):
    """cum: cumulative prices of the case's events at the largest budget, up to its first refusal (the greedy order of every smaller budget starts alike)"""
    base = int(bbal) + 48
    if kind == "bbal + 48: nothing fits" or not cum.size:
        return base
    if kind == "a few bits: nothing fits":
        return base + int(g.integers(1, 60))                               # the cheapest first step is 60 + 2 + 6 bits
    if kind == "exactly the first event":
        return base + int(cum[0])
    if kind == "the largest frame":
        return ALLOC_MAX_ADB
    if kind == "random":
        return int(g.integers(base, ALLOC_MAX_ADB + 1)) if g.integers(0, 2) else int(g.integers(base, min(base + 3000, ALLOC_MAX_ADB) + 1))
    if kind.endswith("k'"):                                                # every cell has stepped the same number of times: the end of a round where all tie
        k = min(int(ncell) * int(g.integers(1, 4)), cum.size)
    else:
        k = int(g.integers(2, cum.size + 1)) if cum.size > 2 else cum.size
    return min(base + int(cum[k - 1]) - (1 if kind.startswith("one bit short") else 0), ALLOC_MAX_ADB)


# the pair call: budgets of unit 0 and unit 1
ALLOC_PAIR_BUDGETS = (("one bit short of the events up to k", "the largest frame"), ("the largest frame", "one bit short of the events up to k"),
                      ("one bit short of the events up to k", "one bit short of the events up to k'"), ("one bit short of the events up to k'", "one bit short of the events up to k"),
                      ("bbal + 48: nothing fits", "the largest frame"), ("the largest frame", "bbal + 48: nothing fits"), ("bbal + 48: nothing fits", "a few bits: nothing fits"),
                      ("exactly the events up to k", "one bit short of the events up to k"), ("exactly the first event", "random"), ("random", "exactly the first event"),
                      ("a few bits: nothing fits", "exactly the events up to k'"), ("the largest frame", "the largest frame"), ("exactly the events up to k", "exactly the events up to k'"),
                      ("random", "one bit short of the events up to k"))


def alloc_set(pair):
    """-> dict(tab, nch, jsb, call [n], adb [n, 2], smr [n, 2, 32], scfsi [n, 2, 32] ([case][ch or unit][sb]), names).  Every table, both nch, every legal
    jsbound; the SMR kinds of ALLOC_SMR_KINDS; budgets placed on the oracle's trace of the same case at the largest budget"""
    key = "alloc%d" % pair
    if key in _args:
        return _args[key]
    T = _alloc_tables()
    g = np.random.default_rng(48 + pair)
    if pair:
        cfgs = [(t, 1, int(T["sblimit"][t])) for t in range(5)] * 3
    else:
        cfgs = [(t, 1, int(T["sblimit"][t])) for t in range(5)] + [(t, 2, j) for t in range(5) for j in sorted({4, 8, 12, 16, int(T["sblimit"][t])})]
    base = []                                                              # (tab, nch, jsb, kind, smr, scfsi)
    for t, nch, jsb in cfgs:
        for kind in ALLOC_SMR_KINDS:
            if kind == "upper channel first" and not (nch == 2 and jsb < T["sblimit"][t]) and not pair:
                kind = "cells at different levels tie"
            base.append((t, nch, jsb, kind) + _alloc_smr(g, kind, t, T))
    arr = lambda i: np.array([b[i] for b in base])
    if pair:                                                               # each unit a mono allocation of its own
        full = [alloc_greedy(arr(0), arr(1), arr(2), np.full(len(base), ALLOC_MAX_ADB), np.stack([arr(4)[:, u], arr(4)[:, u]], axis=1), np.stack([arr(5)[:, u], arr(5)[:, u]], axis=1)) for u in range(2)]
    else:
        full = [alloc_greedy(arr(0), arr(1), arr(2), np.full(len(base), ALLOC_MAX_ADB), arr(4), arr(5))]
    facts = [alloc_facts(R) for R in full]
    _, _, live, joint, bbal = _alloc_geometry(arr(0), arr(1), arr(2))
    ncell = live.sum(axis=(1, 2)) - joint.sum(axis=1)
    cases = []                                                             # (tab, nch, jsb, adb0, adb1, smr, scfsi, name)
    for i, (t, nch, jsb, kind, smr, sel) in enumerate(base):
        cum = [np.cumsum(R["price"][i, :F["free"][i]]) for R, F in zip(full, facts)]
        if pair:
            for k0, k1 in ALLOC_PAIR_BUDGETS:
                cases.append((t, nch, jsb, _alloc_budget(g, k0, bbal[i], cum[0], ncell[i]), _alloc_budget(g, k1, bbal[i], cum[1], ncell[i]), smr, sel, "%s; unit 0: %s, unit 1: %s" % (kind, k0, k1)))
        else:
            for k0 in ALLOC_BUDGETS:
                cases.append((t, nch, jsb, _alloc_budget(g, k0, bbal[i], cum[0], ncell[i]), 0, smr, sel, "%s; %s" % (kind, k0)))
    nmade = len(cases)
    nrandom = 1024
    for _ in range(nrandom):
        t = int(g.integers(0, 5))
        nch = 1 if pair else int(g.integers(1, 3))
        jsb = int(g.choice(sorted({4, 8, 12, 16, int(T["sblimit"][t])}))) if not pair else int(T["sblimit"][t])
        smr, sel = _alloc_smr(g, "random", t, T)
        bb = int(_alloc_geometry(np.array([t]), np.array([nch]), np.array([jsb]))[4][0])
        cases.append((t, nch, jsb, _alloc_budget(g, "random", bb, np.ones(1), 0), _alloc_budget(g, "random", bb, np.ones(1), 0) if pair else 0, smr, sel, "random"))
    col = lambda i, dt: np.array([c[i] for c in cases], dtype=dt)
    S = dict(tab=col(0, I32), nch=col(1, I32), jsb=col(2, I32), call=np.full(len(cases), pair, dtype=I32), adb=np.stack([col(3, I32), col(4, I32)], axis=1),
             smr=col(5, np.float64), scfsi=col(6, I32), names=[c[7] for c in cases], constructed=nmade, random=nrandom)
    assert len(cases) <= 8192
    _args[key] = S
    return S


def alloc_oracle(S):
    """-> (ba per lane [n, 64], bits left [n] (0 for the pair call), the traces: one for tl_allocate, one per unit for tl_allocate_pair).  Made once per set"""
    if "oracle" not in S:
        if S["call"][0]:
            two = lambda x, u: np.stack([x[:, u], x[:, u]], axis=1)
            R = [alloc_greedy(S["tab"], S["nch"], S["jsb"], S["adb"][:, u], two(S["smr"], u), two(S["scfsi"], u)) for u in range(2)]
            ba = np.stack([R[0]["ba"][:, 0], R[1]["ba"][:, 0]], axis=2)   # lane 2 sb + u
            left = np.zeros(S["tab"].size, dtype=np.int64)
        else:
            R = [alloc_greedy(S["tab"], S["nch"], S["jsb"], S["adb"][:, 0], S["smr"], S["scfsi"])]
            ba, left = R[0]["ba"].transpose(0, 2, 1), R[0]["left"]
        S["oracle"] = (ba.reshape(-1, 64), left, R)
    return S["oracle"]


def _alloc_report(S, who, other, c, got_ba, want_ba, got_left, want_left):
    """the case, its table / nch / jsbound / budget, the first differing (channel, subband) with both values"""
    pair = int(S["call"][c])
    head = "%s, %s / %s: case %d (%s): table %d, nch %d, jsbound %d, adb %s" % (
        "tl_allocate_pair" if pair else "tl_allocate", who, other, c, S["names"][c], S["tab"][c], S["nch"][c], S["jsb"][c], S["adb"][c].tolist() if pair else int(S["adb"][c, 0]))
    d = np.flatnonzero(got_ba != want_ba)
    if d.size:
        return "%s: %s %d subband %d: ba %d, want %d (%d cells differ)" % (head, "unit" if pair else "channel", d[0] & 1, d[0] >> 1, got_ba[d[0]], want_ba[d[0]], d.size)
    return "%s: bits left %d, want %d" % (head, got_left, want_left)


def alloc_check(S, out0, out1):
    ba, left, _ = alloc_oracle(S)
    got = out0.reshape(-1, 64)
    bad = np.flatnonzero((got != ba).any(axis=1) | (out1 != left))
    if bad.size:
        c = int(bad[0])
        return _alloc_report(S, "result", "oracle", c, got[c], ba[c], out1[c], left[c]) + " (%d cases differ)" % bad.size
    return None


def alloc_coverage(S):
    """the coverage conditions of the set, from the oracle's traces -> {condition: number of cases}; for the pair call a condition counts where a unit meets it"""
    _, _, R = alloc_oracle(S)
    F = [alloc_facts(r) for r in R]
    names = ["tied", "xlevel", "refused_then_admitted", "left_zero", "nothing", "saturated"] + ([] if S["call"][0] else ["ch1"])
    cover = {k: int(np.any([f[k] for f in F], axis=0).sum()) for k in names}
    if S["call"][0]:
        cover["units_differ"] = int((F[0]["events"] != F[1]["events"]).sum())
        # what the pair call is about: one unit's events stop short while the other's go on / both stop short / one has nothing from the start
        short = [f["refused_then_admitted"] | (~f["saturated"] & ~f["nothing"]) for f in F]
        cover["one_unit_short"] = int((short[0] & F[1]["saturated"] | short[1] & F[0]["saturated"]).sum())
        cover["both_units_short"] = int((short[0] & short[1]).sum())
        cover["one_unit_nothing"] = int((F[0]["nothing"] != F[1]["nothing"]).sum())
    return cover


# ---- running a form
def _form_of(test):
    return STAGE["bits" if test.startswith("put_bits") else "alloc" if test.startswith("alloc") else test]


def run_stage(fn, test):
    """fn = probe_stage of the emulation or tlb_debug_probe_stage of the TEST library -> (rc, S, out0, out1)"""
    f64 = lambda shape: np.full(shape, np.nan)
    if test == "add_db":
        S = add_db_set()
        n, ins, outs = S["a"].size, (S["a"], S["b"], None), (f64(S["a"].size), f64(4 * S["a"].size))
    elif test == "mask":
        S = mask_set()
        n, ins, outs = S["x"].size, (S["x"], S["mb"], S["aux"]), (f64(8 * S["x"].size), f64(5 * S["x"].size))
    elif test == "mnr_key":
        S = mnr_key_set()
        n, ins, outs = S["x"].size, (S["x"], None, None), (np.zeros(S["x"].size, dtype=U64), None)
    elif test == "sf_index":
        v = sf_index_set(scalefactors())
        S = dict(x=v, constructed=v.size - 800000, random=800000)
        n, ins, outs = v.size, (v, None, None), (np.full(2 * v.size, -1, dtype=I32), np.full(v.size, -1, dtype=I32))
    elif test == "div_by":
        S = div_by_set()
        n, ins, outs = S["s"].size, (S["s"], S["d"], None), (f64(S["s"].size), f64(S["s"].size))
    elif test == "spans":
        S = spans_set()
        n = S["list"].shape[0]
        ins, outs = (S["list"], S["bounds"], S["counts"]), (np.full(512 * n, -9, dtype=I32), np.full(2 * n, -9, dtype=I32))
    elif test == "min_rows":
        S = min_rows_set()
        n = S["col"].shape[0]
        ins, outs = (S["col"], S["m"], S["rows"]), (f64(64 * n), None)
    elif test.startswith("alloc"):
        S = alloc_set(1 if test == "alloc_pair" else 0)
        n = S["tab"].size
        par = np.zeros((n, 8), dtype=I32)
        par[:, 0], par[:, 1], par[:, 2], par[:, 3], par[:, 4:6] = S["tab"], S["nch"], S["jsb"], S["call"], S["adb"]
        ins = (S["smr"].transpose(0, 2, 1), S["scfsi"].transpose(0, 2, 1), par)             # lane = 2 sb + ch (or unit)
        outs = (np.full(64 * n, -9, dtype=I32), np.full(n, -9, dtype=I32))
    else:
        S = bits_set(1 if test == "put_bits48" else 0)
        n = S["val"].shape[0]
        ins, outs = (S["val"], S["len"], S["par"]), (np.full(3 * FRAME_WORDS * n, 0xdeadbeef, dtype=np.uint32), np.full(128 * n, 0xdeadbeef, dtype=np.uint32))
    form = _form_of(test)
    ins = [None if x is None else np.ascontiguousarray(x) for x in ins]
    rc = fn(form, n, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), _ptr(outs[0]), _ptr(outs[1]))
    return rc, S, outs[0], outs[1]


def stage_check(test, S, out0, out1):
    """a run's outputs against the form's oracle -> None, or a message naming form, argument and both results"""
    tab = _emu_tables()[0]
    if test == "add_db":
        msg = add_db_check(S, out0, out1, tab=tab)
        if msg is None:                                                    # the far level leaves the other operand's bits
            sb, sa = S["far"]
            if same_bits(out0[sb], S["a"][sb]).size or same_bits(out0[sa], S["b"][sa]).size:
                msg = "tl_add_db: a sum with the far level is not the other operand"
        return msg
    if test == "mask":
        return mask_check(S, out0, out1, tab)
    if test == "spans":
        return spans_check(S, out0, out1)
    if test == "min_rows":
        return min_rows_check(S, out0)
    if test == "mnr_key":
        return mnr_key_check(S, out0)
    if test == "sf_index":
        return sf_index_check(S["x"], scalefactors(), out0, out1)
    if test == "div_by":
        return div_by_check(S, out0, out1)
    if test.startswith("alloc"):
        return alloc_check(S, out0, out1)
    return bits_check(S, out0, out1)


def stage_same(test, S, dev, emu_out):
    """device == emulation, every word of both outputs -> None or a message naming the first argument / case that differs and both results"""
    per = {"add_db": (1, 4), "mask": (8, 5), "mnr_key": (1, 0), "sf_index": (2, 1), "div_by": (1, 1), "spans": (512, 2), "min_rows": (64, 0),
           "put_bits": (3 * FRAME_WORDS, 128), "put_bits48": (3 * FRAME_WORDS, 128), "alloc": (64, 1), "alloc_pair": (64, 1)}[test]
    raw = lambda x: x.view(U64) if x.dtype == np.float64 else x
    if test.startswith("alloc"):                                          # the case, its parameters and the first differing cell
        d, e = dev[0].reshape(-1, 64), emu_out[0].reshape(-1, 64)
        bad = np.flatnonzero((d != e).any(axis=1) | (dev[1] != emu_out[1]))
        if bad.size:
            c = int(bad[0])
            return _alloc_report(S, "device", "emulation", c, d[c], e[c], dev[1][c], emu_out[1][c]) + " (%d cases differ)" % bad.size
        return None
    for k in range(2):
        if dev[k] is None:
            continue
        bad = np.flatnonzero(raw(dev[k]) != raw(emu_out[k]))
        if bad.size:
            i, j = divmod(int(bad[0]), per[k])
            return "%s, device / emulation: output %d, %s %d, word %d: device %#x, emulation %#x (%d words differ)" % (
                test, k, "argument" if _form_of(test) < 5 else "case", i, j, int(raw(dev[k])[bad[0]]), int(raw(emu_out[k])[bad[0]]), bad.size)
    return None


def _stage_call(fn, form, n, *arrs):
    arrs = [None if x is None else np.ascontiguousarray(x) for x in arrs]
    return fn(form, n, *[_ptr(x) for x in arrs])


def check_stage_argument_checks(fn):
    """what the stage probe refuses with TLB_ERR_ARG before anything is queued: one argument outside each form's domain, an unknown form, n = 0, a
    missing pointer -- and a good call afterwards returns the right values"""
    d = lambda *v: np.array(v, dtype=np.float64)
    o = lambda k: np.zeros(k)
    good_a, good_b = d(1.0, 2.0, 3.0), d(0.0, -5.0, 2.5)
    call = lambda form, n, *a: _stage_call(fn, STAGE[form], n, *a)
    assert call("add_db", 3, d(1.0, np.nan, 3.0), good_b, None, o(3), o(12)) == ERR_ARG                         # a NaN operand
    assert call("add_db", 3, good_a, d(0.0, 2.0 ** 19, 1.0), None, o(3), o(12)) == ERR_ARG                      # a dB operand of 2^19
    assert call("add_db", 3, good_a, d(0.0, -np.inf, 1.0), None, o(3), o(12)) == ERR_ARG
    aux = np.array([[10.0, 0.0, 1.0, 1.0]] * 3)
    assert call("mask", 3, good_a, d(1.0, 32.5, 3.0), aux, o(24), o(15)) == ERR_ARG                             # a bark above 32
    assert call("mask", 3, good_a, d(1.0, -0.5, 3.0), aux, o(24), o(15)) == ERR_ARG
    bad_aux = aux.copy(); bad_aux[2, 2] = 0.5
    assert call("mask", 3, good_a, good_a, bad_aux, o(24), o(15)) == ERR_ARG                                    # tonal is 0 or 1
    bad_aux = aux.copy(); bad_aux[1, 0] = np.nan
    assert call("mask", 3, good_a, good_a, bad_aux, o(24), o(15)) == ERR_ARG
    assert call("mnr_key", 3, d(1.0, np.nan, 2.0), None, None, np.zeros(3, dtype=U64), None) == ERR_ARG
    assert call("sf_index", 3, d(1.0, 2.0, 0.5), None, None, np.zeros(6, dtype=I32), np.zeros(3, dtype=I32)) == ERR_ARG        # cur_max < 2
    assert call("sf_index", 3, d(1.0, -1e-9, 0.5), None, None, np.zeros(6, dtype=I32), np.zeros(3, dtype=I32)) == ERR_ARG
    assert call("div_by", 3, good_a, d(1.0, 0.0, 3.0), None, o(3), o(3)) == ERR_ARG                             # no divisor of the encoder
    assert call("div_by", 3, good_a, d(1.0, float(np.nextafter(2.0, 0.0)), 3.0), None, o(3), o(3)) == ERR_ARG   # a significand of all ones: Markstein's exception
    assert call("div_by", 3, d(1.0, 1e300, 3.0), good_a, None, o(3), o(3)) == ERR_ARG
    lst, bnd = np.tile(np.linspace(0.0, 24.0, LIST), (2, 1)), np.tile(d(2.0, 13.0), (2, 64, 1))
    so, sf_ = np.zeros(1024, dtype=I32), np.zeros(4, dtype=I32)
    assert call("spans", 2, lst, bnd, np.array([[3, 4], [65, 64]], dtype=I32), so, sf_) == ERR_ARG               # ntone + nnoise = 129
    assert call("spans", 2, lst, bnd, np.array([[3, 4], [-1, 4]], dtype=I32), so, sf_) == ERR_ARG
    bad_lst = lst.copy(); bad_lst[1, 5] = np.nan
    assert call("spans", 2, bad_lst, bnd, np.array([[3, 4], [10, 4]], dtype=I32), so, sf_) == ERR_ARG
    col, m = np.zeros((2, ROWS)), np.zeros((2, 64))
    rows = np.tile(np.array([0, 4, 1], dtype=I32), (2, 64, 1))
    bad_rows = rows.copy(); bad_rows[1, 63] = (130, 7, 0)                                                       # rows [130, 137): past the column
    assert call("min_rows", 2, col, m, bad_rows, o(128), None) == ERR_ARG
    bad_rows = rows.copy(); bad_rows[0, 1] = (3, 0, 0)
    assert call("min_rows", 2, col, m, bad_rows, o(128), None) == ERR_ARG
    val, ln = np.zeros((2, 64, FIELDS), dtype=U64), np.full((2, 64, FIELDS), 30, dtype=I32)
    bo, bc = np.zeros(2 * 3 * FRAME_WORDS, dtype=np.uint32), np.zeros(256, dtype=np.uint32)
    par = np.array([[0, 0], [0, 0]], dtype=I32)
    assert call("bits", 2, val, np.full((2, 64, FIELDS), 48, dtype=I32), np.array([[0, 1], [0, 1]], dtype=I32), bo, bc) == ERR_ARG      # 18432 bits: a field runs past the frame
    bad_ln = ln.copy(); bad_ln[1, 7, 2] = 33
    assert call("bits", 2, val, bad_ln, par, bo, bc) == ERR_ARG                                                 # tl_put_bits takes 0..32
    bad_val = val.copy(); bad_val[0, 0, 0] = U64(1) << U64(30)
    assert call("bits", 2, bad_val, ln, par, bo, bc) == ERR_ARG                                                 # a value wider than its field
    assert call("bits", 2, val, ln, np.array([[0, 0], [64, 0]], dtype=I32), bo, bc) == ERR_ARG
    # the allocation: one case outside each rule of its domain beside a good one
    asmr, asel = np.zeros((2, 64)), np.zeros((2, 64), dtype=I32)
    apar = np.array([[0, 2, 27, 0, 3000, 0, 0, 0], [4, 1, 30, 1, 2000, 1500, 0, 0]], dtype=I32)
    ao, al = np.zeros(128, dtype=I32), np.zeros(2, dtype=I32)

    def alloc_with(case, **kw):
        par, smr, sel = apar.copy(), asmr.copy(), asel.copy()
        for k, v in kw.items():
            if k == "smr":
                smr[case, 17] = v
            elif k == "scfsi":
                sel[case, 40] = v
            else:
                par[case, {"tab": 0, "nch": 1, "jsb": 2, "call": 3, "adb": 4, "adb1": 5}[k]] = v
        return call("alloc", 2, smr, sel, par, ao, al)
    assert alloc_with(0) == 0
    assert alloc_with(0, tab=5) == ERR_ARG and alloc_with(1, tab=-1) == ERR_ARG                                 # tables 0..4
    assert alloc_with(0, nch=3) == ERR_ARG and alloc_with(0, nch=0) == ERR_ARG
    assert alloc_with(1, nch=2) == ERR_ARG                                                                      # the pair call is two MONO streams
    assert alloc_with(0, call=2) == ERR_ARG
    assert alloc_with(0, jsb=5) == ERR_ARG and alloc_with(0, jsb=30) == ERR_ARG                                 # 4, 8, 12, 16 or the table's sblimit (27)
    assert alloc_with(0, jsb=16) == 0
    assert alloc_with(1, scfsi=4) == ERR_ARG and alloc_with(0, scfsi=-1) == ERR_ARG
    assert alloc_with(0, smr=np.nan) == ERR_ARG and alloc_with(1, smr=1000.5) == ERR_ARG and alloc_with(0, smr=-np.inf) == ERR_ARG
    assert alloc_with(0, adb=100) == ERR_ARG                                                                    # below bbal + 48: a negative budget
    assert alloc_with(0, adb=ALLOC_MAX_ADB + 1) == ERR_ARG
    assert alloc_with(1, adb1=75 + 47) == ERR_ARG and alloc_with(1, adb1=75 + 48) == 0                          # unit 1's budget too (table 4 mono: bbal = 75)
    p = o(16)
    q = _ptr(p)
    assert fn(-1, 2, q, q, q, q, q) == ERR_ARG and fn(STAGE_NFORMS, 2, q, q, q, q, q) == ERR_ARG                # an unknown form
    assert fn(0, 0, q, q, q, q, q) == ERR_ARG and fn(0, -3, q, q, q, q, q) == ERR_ARG                           # n = 0
    assert fn(0, 2, None, q, q, q, q) == ERR_ARG and fn(0, 2, q, None, q, q, q) == ERR_ARG and fn(0, 2, q, q, q, None, q) == ERR_ARG and fn(0, 2, q, q, q, q, None) == ERR_ARG
    assert fn(STAGE["mask"], 2, q, q, None, q, q) == ERR_ARG and fn(STAGE["spans"], 1, q, q, None, q, q) == ERR_ARG
    # ... and a good call after all that returns the right values
    o0, o1 = o(3), o(12)
    assert call("add_db", 3, d(10.0, 0.0, -300.0), d(10.0, 150.0, 5.0), None, o0, o1) == 0
    tab = _emu_tables()[0]
    assert o0.tolist() == [10.0 + tab[0], 150.0, 5.0] and o1.reshape(3, 4)[:, 0].tolist() == o0.tolist()
    k = np.zeros(2, dtype=U64)
    assert call("mnr_key", 2, d(0.0, 1e6), None, None, k, None) == 0 and k.tolist() == [1 << 63, (1 << 64) - 1]
