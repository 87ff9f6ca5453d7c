"""The FP8 weight form of csrc/gemm_w8.hip, restated with NumPy / torch on the CPU: the
quantiser (row exponent, e4m3 round-to-nearest-even, twin), the packed layout, the K split
cs_gemm_bf16_w8 picks, and the exact GPU cases.  tests/test_w8_host.py checks this file
(against torch.float8_e4m3fn among others), the test_w8_*_gpu.py files check the kernels
against it.

Format: OCP e4m3fn, 1 sign, 4 exponent (bias 7), 3 mantissa bits; exponent field 0 is the
subnormal grid m * 2^-9; 0x7f / 0xff are NaN; the largest finite value is 448 (0x7e).
  e[n]       = the smallest integer with amax_n * 2^-e[n] <= 448 (an all-zero row: 0)
  code[n][k] = e4m3_rne(w[n][k] * 2^-e[n])
  twin[n][k] = value(code[n][k]) * 2^e[n]
All arithmetic here is fp64: bf16 inputs, powers of two and code values are exact in it."""
import functools
import math

import numpy as np
import torch

import gemm_ref as R

MAX_ROWS = 80                 # cs_gemm_w8_max_rows()
BN = 128                      # W rows per workgroup
MAX_SPLITS = 16
STATUS_NONFINITE, STATUS_ROW_RANGE = 1, 2
FINITE_CODES = np.array([c for c in range(256) if c & 0x7f != 0x7f], dtype=np.uint8)


def code_value(code):
    """value(code) as fp64 (NaN codes: nan)."""
    code = np.asarray(code, dtype=np.int64)
    m, ef = code & 7, (code >> 3) & 15
    v = np.where(ef == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (ef - 10.0))
    v = np.where(code & 0x7f == 0x7f, np.nan, v)
    return np.where(code & 0x80, -v, v)


_POS = code_value(np.arange(0x7f))         # the 127 non-negative finite values, ascending


def encode_rne(q):
    """e4m3_rne(q) for fp64 |q| <= 448: round to the nearest grid point, ties to the even
    mantissa; the sign of zero is kept."""
    q = np.asarray(q, dtype=np.float64)
    a = np.abs(q)
    assert bool((a <= 448).all())
    ex = np.floor(np.log2(np.maximum(a, 2.0 ** -6)))      # the binade (subnormals: that of 2^-6)
    step = 2.0 ** (ex - 3)
    r = np.rint(a / step) * step                         # np.rint rounds half to even
    code = np.searchsorted(_POS, r).astype(np.int64)
    assert bool((_POS[code] == r).all())
    return (code | np.where(np.signbit(q), 0x80, 0)).astype(np.uint8)


def row_exponent(amax):
    """The smallest integer e with amax * 2^-e <= 448; 0 for amax == 0."""
    if amax == 0:
        return 0
    f, x = math.frexp(float(amax))          # amax = f 2^x, f in [0.5, 1); 448 = 0.875 * 2^9
    return x - 9 if f <= 0.875 else x - 8


def quantise(w):
    """w bf16 [N, K] -> (codes uint8 [N, K], exps int64 [N], twin bf16 [N, K], status): what
    cs_gemm_w8_pack computes.  status != 0: the outputs are what the kernel would NOT write."""
    assert w.dtype == torch.bfloat16 and w.dim() == 2
    w64 = w.double().numpy()
    status = 0
    if not np.isfinite(w64).all():
        return None, None, None, STATUS_NONFINITE
    exps = np.array([row_exponent(a) for a in np.abs(w64).max(axis=1)], dtype=np.int64)
    if (exps < -128).any() or (exps > 127).any():
        status |= STATUS_ROW_RANGE
    codes = encode_rne(w64 * 2.0 ** -exps[:, None].astype(np.float64))
    t64 = code_value(codes) * 2.0 ** exps[:, None].astype(np.float64)
    with np.errstate(over="ignore"):
        twin = torch.from_numpy(t64).to(torch.float32).to(torch.bfloat16)
    if not np.array_equal(twin.double().numpy(), t64):       # overflow, or below bf16's grid
        status |= STATUS_ROW_RANGE
    return codes, exps, twin, status


def twin_of(codes, exps):
    """value(code) * 2^e as fp64 [N, K]."""
    return code_value(codes) * 2.0 ** np.asarray(exps, dtype=np.float64)[:, None]


# --- the packed layout ---------------------------------------------------------------------------

def packed_index(N, K):
    """idx [N, K]: code[n][k] sits at byte idx[n][k] of codes_packed.  With T = n / 16, r = n % 16,
    s = k / 64, h = k % 64 / 32, g = k % 32 / 8, j = k % 8 and lane l = 16 g + r:
    idx = (T * K / 64 + s) * 1024 + 16 l + 8 h + j."""
    n = np.arange(N, dtype=np.int64)[:, None]
    k = np.arange(K, dtype=np.int64)[None, :]
    T, r = n // 16, n % 16
    s, h, g, j = k // 64, k % 64 // 32, k % 32 // 8, k % 8
    return (T * (K // 64) + s) * 1024 + 16 * (16 * g + r) + 8 * h + j


def pack(codes):
    N, K = codes.shape
    out = np.empty(N * K, dtype=np.uint8)
    out[packed_index(N, K).ravel()] = np.asarray(codes).ravel()
    return out


def unpack(packed, N, K):
    return np.asarray(packed)[packed_index(N, K)]


# --- the host half -------------------------------------------------------------------------------

def splits(M, N, K, gated=False):
    """cs_gemm_w8_splits"""
    if M <= 0 or N <= 0 or K <= 0 or N % BN or K % R.BK:
        return 0
    if gated:
        return 1
    tiles, s = N // BN, 1
    while tiles * s < 256 and s * 2 <= MAX_SPLITS and K % (R.BK * s * 2) == 0 and K // (R.BK * s * 2) >= 8:
        s *= 2
    return s


# --- the exact GPU cases -------------------------------------------------------------------------

# the row tiles are 16 rows: every tile count full and one row into the next, up to max_rows
CASE_M = (1, 16, 17, 32, 33, 48, 49, 64, 65, 80)
CASE_N = (512, 384)
ZERO_STEPS = R.ZERO_STEPS + (32,)     # splits = 0: the library picks 1, 2, 2, 4 at these N
ROW_E = (-20, 0, 20)                  # exponent of row n: ROW_E[n % 3]
GATED_E = -10
MAX_STEPS = max(R.THIN_MAX_STEPS, R.MAX_STEPS, max(ZERO_STEPS))


def case_shapes(gated):
    """(nk, splits): K = 64 nk max(splits, 1).  The register ring is 6 steps deep with a tail of
    up to 5: NK and THIN_NSTEPS give nk % 6 = 1, 2, 3, 4, 5, 1, 1, 2, 3, 5, 1, 3, 1 and zero to
    eight whole rings."""
    one = sorted(set(R.NK) | set(R.THIN_NSTEPS))
    if gated:
        return [(nk, 1) for nk in one]
    return [(nk, 1) for nk in one] + [(nk, s) for nk in R.NK for s in (2, 3)] + \
        [(n, 0) for n in ZERO_STEPS]


def case_seed(M, N):
    return 8800 + M + N


def case_operands(M, N):
    """gemm_ref.operands at the w8 cases' length: integers |v| <= 15, exact as e4m3 codes."""
    return R.operands(M, N, MAX_STEPS, case_seed(M, N))


def case_prefix(M, N):
    return R.prefix_products(M, N, MAX_STEPS, case_seed(M, N))


def case_exps(N, gated):
    e = np.full(N, GATED_E, dtype=np.int64) if gated else np.array(ROW_E, dtype=np.int64)[np.arange(N) % 3]
    return e


def scale_rows(v64, exps):
    """v [.., N] fp64 times 2^e[n]"""
    return v64 * torch.from_numpy(2.0 ** np.asarray(exps, dtype=np.float64))


def every_code_matrix(N, K):
    """codes [N, K] = the finite code number (131 n + 7 k) mod 254: 131 and 7 are coprime to
    254, so every column of N >= 254 rows (and every row of K >= 254) holds all 254 codes."""
    n = np.arange(N, dtype=np.int64)[:, None]
    k = np.arange(K, dtype=np.int64)[None, :]
    return FINITE_CODES[(131 * n + 7 * k) % 254]
