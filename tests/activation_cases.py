"""The specification of the six element-wise kinds that call the device's erff / tanhf / expm1f / expf / log1pf
(CBPointwise2d(transcendental=True), cb_pointwise.hip): each kind's formula in float64, and the bound
the kernel's float32 evaluation of it must keep.  There is no bit-for-bit twin for these kinds, as there is none for
SIGMOID / SILU / TANH.  Shapes, mask patterns, values and the mask layout are tests/pointwise_cases.py's.

The float64 formula uses the float32-ROUNDED constants and parameters the kernel uses, so that the bound covers the
evaluation alone; SOFTPLUS's branch is taken on the float32 product fl(v p0), as the kernel takes it.

THE BOUNDS, in units of 2^-24 (half an ulp of a float32 result: what one correctly rounded operation adds, relative to
its result).  The device functions' limits are those of the OpenCL full profile, which OCML is built to, TAKEN TWICE,
an ulp being two units: erf 16 ulp -> 64 units, exp 3 -> 12, expm1 3 -> 12, log1p 2 -> 8, tanh 5 -> 20.  An error of a
function's argument enters its result through the condition number |x f'(x) / f(x)|; to first order (the products of
two such terms are below 2^-40 and lie inside the doubling).  Every operation written counts one unit, also where it
happens to be exact (0.5 v, a product with p1 = 1).

  GELU       0.5 v (1 + erf(u)), u = v k.  u: 1 unit, which enters erf as |u erf'(u)| = (2 / sqrt(pi)) |u| exp(-u^2)
             <= 0.484 in ABSOLUTE terms; erff: 64 units of |erf(u)| <= 1.  So the error of e = erff(u) is at most 64.484
             units absolute -- and 1 + e cancels for negative v, so this error reaches the result as 0.5 |v| 64.484
             units whatever |ref| is: a = 33.  Relative to the result: the sum 1 + e, the product 0.5 v, the last
             product: b = 3.                                     |err| <= (33 |v| + 3 |ref|) 2^-24
  GELU_TANH  0.5 v (1 + tanh(z)), z = c0 (v + c1 v^3).  v v, (v v) v, c1 (..): 3 units on m = c1 v^3; w = v + m: m and
             v have one sign, so |m| <= |w| and w carries 3 + 1 = 4; z = c0 w: 5 units, entering tanh as
             5 |z| sech^2(z) <= 5 * 0.448 = 2.24 absolute; tanhf: 20 units of |tanh| <= 1: 22.24 absolute, times
             0.5 |v|: a = 12.  b = 3 as above.                   |err| <= (12 |v| + 3 |ref|) 2^-24
  ELU        v > 0: v itself, no error.  Else p0 expm1(t), t = v p1: 1 unit on t, through expm1's condition number
             t e^t / (e^t - 1), which is <= 1 for t <= 0 (and <= 1 + t for t > 0, a negative p1); expm1f 12; the
             product 1.                                          c = 14  (13 + 1 + t for t > 0)
  SELU       v > 0: one product, c = 1.  Else expm1f of the exact v, 12, and the product.           c = 13
  SOFTPLUS   t > p1: v itself.  Else log1p(exp(t)) / p0: expf 12 units, through log1p's condition number
             E / ((1 + E) log1p(E)) <= 1; log1pf 8; the division 1: 21.  For p0 != 1 the one unit of t = v p0 enters
             through the whole function's condition number |t| sigmoid(t) / softplus(t), which is <= 1 for t >= 0 and
             approaches |t| for very negative t (it is <= |t| there: log(1 + y) >= y / (1 + y)).
                                                                 c = 21, for p0 != 1 plus max(1, |t|)
  MISH       v tanh(log1p(exp(v))): expf 12 (v is exact); log1pf 8 + 12 (condition <= 1, as above); tanhf 20 + 20 (its
             condition number 2 L / sinh(2 L) <= 1); the product 1.                                 c = 41

Every bound gets + 2^-126 (the smallest normal float32); an fp16 map adds the one rounding to f16, 2^-11 |ref| + 2^-24
(2^-24 its smallest subnormal).  The constants are derived, not tuned: a failure is a finding.

No GPU is needed to import this file."""
import numpy as np
import torch

from pointwise_cases import SHAPES, FORMS, bits_of, pack, patterns, values      # noqa: F401  (shared with the tests)

F32 = np.float32
(GELU, GELU_TANH, ELU, SELU, SOFTPLUS, MISH) = range(16, 22)
NAMES = {GELU: "GELU", GELU_TANH: "GELU_TANH", ELU: "ELU", SELU: "SELU", SOFTPLUS: "SOFTPLUS", MISH: "MISH"}
# (kind, p0, p1) of the bound tests; p1 of the third ELU is CELU(1.3)'s: 1 / alpha rounded to float32
CASES = [(GELU, 0.0, 0.0), (GELU_TANH, 0.0, 0.0), (ELU, 1.0, 1.0), (ELU, 0.5, 2.0), (ELU, 1.3, float(F32(1.0 / 1.3))),
         (SELU, 0.0, 0.0), (SOFTPLUS, 1.0, 20.0), (SOFTPLUS, 2.0, 5.0), (MISH, 0.0, 0.0)]
# inputs of the bound tests besides the uniform ones in [-20, 20]
SPECIAL = [np.inf, -np.inf, np.nan, 20.0, -20.0, 0.0, -0.0]

# the kernel's constants as written: sqrt(1/2), sqrt(2/pi), GELU's cubic coefficient, SELU's scale and alpha scale
CONSTANTS = (0.70710678118654752440, 0.79788456080286535588, 0.044715, 1.0507009873554805, 1.7580993408473766)

UNIT = 2.0 ** -24


def case_name(kind, p0, p1):
    return NAMES[kind] + ("(%g, %g)" % (p0, p1) if kind in (ELU, SOFTPLUS) else "")


def _erf(u):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(u))).numpy()


def reference64(x, kind, p0=0.0, p1=0.0, rounded=True):
    """The kind's formula on x (float32 or float16, no affine) in float64, with the float32-rounded constants and
    parameters -- rounded=False: with the constants as written, which is torch's operator in double."""
    v = x.astype(np.float64)
    K_SQRT_HALF, K_SQRT_2_PI, K_CUBIC, K_SELU_SCALE, K_SELU_ALPHA_SCALE = (
        float(F32(k)) if rounded else k for k in CONSTANTS)
    p0, p1 = float(F32(p0)), float(F32(p1))
    with np.errstate(all='ignore'):
        if kind == GELU:
            return 0.5 * v * (1.0 + _erf(v * K_SQRT_HALF))
        if kind == GELU_TANH:
            return 0.5 * v * (1.0 + np.tanh(K_SQRT_2_PI * (v + K_CUBIC * (v * v * v))))
        if kind == ELU:
            return np.where(v > 0, v, p0 * np.expm1(v * p1))
        if kind == SELU:
            return np.where(v > 0, K_SELU_SCALE * v, K_SELU_ALPHA_SCALE * np.expm1(v))
        if kind == SOFTPLUS:
            t32 = x.astype(F32) * F32(p0)      # (the branch as the kernel takes it)
            return np.where(t32 > F32(p1), v, np.log1p(np.exp(v * p0)) / p0)
        assert kind == MISH
        return v * np.tanh(np.log1p(np.exp(v)))


def bound(x, ref, kind, p0=0.0, p1=0.0):
    """The bound on |kernel - ref| at the finite entries of ref, derived in this file's docstring; x's dtype is the
    map's."""
    v = x.astype(np.float64)
    mag = np.abs(ref)
    p0, p1 = float(F32(p0)), float(F32(p1))
    with np.errstate(all='ignore'):
        if kind == GELU:
            b = (33.0 * np.abs(v) + 3.0 * mag) * UNIT
        elif kind == GELU_TANH:
            b = (12.0 * np.abs(v) + 3.0 * mag) * UNIT
        elif kind == ELU:
            t = v * p1
            b = np.where(v > 0, 0.0, 13.0 + np.where(t > 0, 1.0 + t, 1.0)) * UNIT * mag
        elif kind == SELU:
            b = np.where(v > 0, 1.0, 13.0) * UNIT * mag
        elif kind == SOFTPLUS:
            t = v * p0
            c = 21.0 + (np.maximum(1.0, np.abs(t)) if p0 != 1.0 else 0.0)
            b = np.where(x.astype(F32) * F32(p0) > F32(p1), 0.0, c) * UNIT * mag
        else:
            assert kind == MISH
            b = 41.0 * UNIT * mag
    b = np.where(np.isfinite(b), b, 0.0) + 2.0 ** -126
    if x.dtype == np.float16:
        b = b + 2.0 ** -11 * mag + 2.0 ** -24
    return b


def judge(x, got, kind, p0=0.0, p1=0.0):
    """(ok, worst err / bound, worst err / |ref| where |ref| >= 2^-14, text of the first offenders): `got` against the
    float64 formula on x.  Where the reference is not finite the result must be the same infinity or a NaN."""
    ref = reference64(x, kind, p0, p1)
    g = got.astype(np.float64)
    fin = np.isfinite(ref)
    inf = ~fin & ~np.isnan(ref)
    if not (np.array_equal(np.isnan(g), np.isnan(ref)) and np.array_equal(g[inf], ref[inf])):
        bad = (np.isnan(g) != np.isnan(ref)) | (inf & (g != ref))
        return False, np.inf, np.inf, "non-finite: x %s got %s ref %s" % (x[bad][:4], g[bad][:4], ref[bad][:4])
    err, b, mag = np.abs(g[fin] - ref[fin]), bound(x, ref, kind, p0, p1)[fin], np.abs(ref[fin])
    ratio = float((err / b).max()) if err.size else 0.0
    big = mag >= 2.0 ** -14      # (relative figures where an f16 result is a normal number too)
    rel = float((err[big] / mag[big]).max()) if big.any() else 0.0
    bad = err > b
    text = "%d over the bound: x %s got %s ref %s, worst err / bound %.3f" % (
        int(bad.sum()), x[fin][bad][:4], g[fin][bad][:4], ref[fin][bad][:4], ratio)
    return not bad.any(), ratio, rel, text
