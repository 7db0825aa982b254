/* TEST-ONLY: this machine's libm over arrays -- the reference of tests/test_probe_emu.py / test_probe_gpu.py.
 * gcc -O1 -fno-builtin -ffp-contract=off ... -lm (tests/probelib.py): every call below is a call into libm.so.6, every / one division. */
#define _GNU_SOURCE
#include <math.h>
void ref_log(long n, const double *a, double *r) { for (long i = 0; i < n; i++) r[i] = log(a[i]); }
void ref_log10(long n, const double *a, double *r) { for (long i = 0; i < n; i++) r[i] = log10(a[i]); }
void ref_exp(long n, const double *a, double *r) { for (long i = 0; i < n; i++) r[i] = exp(a[i]); }
void ref_pow10(long n, const double *a, double *r) { for (long i = 0; i < n; i++) r[i] = pow(10.0, a[i]); }
void ref_sincos(long n, const double *a, double *s, double *c) { for (long i = 0; i < n; i++) sincos(a[i], &s[i], &c[i]); }
void ref_atan2(long n, const double *y, const double *x, double *r) { for (long i = 0; i < n; i++) r[i] = atan2(y[i], x[i]); }
void ref_sqrt(long n, const double *a, double *r) { for (long i = 0; i < n; i++) r[i] = sqrt(a[i]); }
void ref_div(long n, const double *a, const double *b, double *r) { for (long i = 0; i < n; i++) r[i] = a[i] / b[i]; }
void ref_fma(long n, const double *a, const double *b, double k, double *r) { for (long i = 0; i < n; i++) r[i] = fma(a[i], b[i], k); }
