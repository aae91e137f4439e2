"""Extended-precision reference for the fp64 MFMA GEMM core (gemm_f64.hip): a plain NumPy transcription of every epilogue's
definition (the comments of enum Epi and GemmDesc in csrc/kernels.hpp), computed in np.longdouble (64-bit mantissa), on LOGICAL
operands -- layouts, leading dimensions and batch strides are the test's business (pack / Packed below), never the reference's.

Logical operands carry the two batch levels in front: A (b2, b1, M, K), B (b2, b1 | 1, K, N), C0 (b2, b1, M, N),
D (b2, b1, ceil(M / rdiv), N), colscale (b2, b1, N), rowscale (b2, ceil(M / rdiv)), kscale (b2, b1, K).
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53

EPI_STORE, EPI_DIV_D, EPI_QUAD, EPI_ACCUM, EPI_GRAD, EPI_DUAL_INIT, EPI_SUB = 0, 1, 2, 3, 4, 6, 7
EPI_NAME = {EPI_STORE: "store", EPI_DIV_D: "div_d", EPI_QUAD: "quad", EPI_ACCUM: "accum", EPI_GRAD: "grad", EPI_SUB: "sub"}
CFG_TILE = {1: 128, 2: 64, 3: 64, 5: 32}          # block tile edge B
CFG_BK = {1: 16, 2: 8, 3: 16, 5: 64}              # K depth


def auto_cfg(M, N, K, batch=1):
    """The launcher's own choice for cfg = 0 (gemm_auto_cfg)."""
    tiles = -(-M // 64) * -(-N // 64) * max(batch, 1)
    return (2 if K <= 320 else 3) if tiles >= 512 else 5


class Ref:
    """C / C2 / C3: longdouble (b2, b1, M, N) or None; quad: longdouble (b2, 1 | 2) or None; the *_mag twins are the magnitudes
    the error bounds are relative to (|alpha| |A||B| times the absolute epilogue factor, plus |C0| where C is read)."""
    C = C2 = C3 = quad = None
    C_mag = C2_mag = C3_mag = quad_mag = None
    n_terms = 0


def _rows(X, rdiv, M):
    """(.., ceil(M / rdiv), N) -> (.., M, N): row i of the result is row i // rdiv."""
    return np.repeat(X, rdiv, axis=-2)[..., :M, :]


def reference(epi, A, B, alpha=1.0, C0=None, D=None, rdiv=1, colscale=None, rowscale=None, kscale=None, want_c2=True, want_c3=True):
    A, B = np.asarray(A, dtype=LD), np.asarray(B, dtype=LD)
    M = A.shape[-2]
    if kscale is not None:                          # C = (A diag(kscale)) B
        A = A * np.asarray(kscale, dtype=LD)[..., None, :]
    acc = np.matmul(A, B)
    mag = np.matmul(np.abs(A), np.abs(B))
    r = Ref()
    if epi == EPI_STORE:                            # C = alpha * acc [* colscale[col]]
        f = LD(alpha) if colscale is None else LD(alpha) * np.asarray(colscale, dtype=LD)[..., None, :]
        r.C, r.C_mag = f * acc, np.abs(f) * mag
    elif epi == EPI_ACCUM:                          # C += alpha * acc
        C0 = np.asarray(C0, dtype=LD)
        r.C, r.C_mag = C0 + LD(alpha) * acc, np.abs(C0) + abs(LD(alpha)) * mag
    elif epi == EPI_SUB:                            # C = C - acc
        C0 = np.asarray(C0, dtype=LD)
        r.C, r.C_mag = C0 - acc, np.abs(C0) + mag
    elif epi in (EPI_DIV_D, EPI_QUAD, EPI_GRAD):
        Dr = _rows(np.asarray(D, dtype=LD), rdiv, M)            # D[(row / rdiv) * ldd + col], the reciprocals
        b, bmag = acc * Dr, mag * np.abs(Dr)
        if epi == EPI_DIV_D:                        # C = acc * D
            r.C, r.C_mag = b, bmag
        elif epi == EPI_QUAD:                       # sum of acc^2 * D per outer entry
            r.quad = np.sum(acc * acc * Dr, axis=(1, 2, 3))[:, None]
            r.quad_mag = np.sum(mag * mag * np.abs(Dr), axis=(1, 2, 3))[:, None]
        else:                                       # C = b, C2 = b * colscale[col], C3 = b * rowscale[row / rdiv]; sums of acc*b, b*b
            r.C, r.C_mag = b, bmag
            if want_c2:
                cs = np.asarray(colscale, dtype=LD)[..., None, :]
                r.C2, r.C2_mag = b * cs, bmag * np.abs(cs)
            if want_c3:
                rs = np.repeat(np.asarray(rowscale, dtype=LD), rdiv, axis=-1)[..., :M][:, None, :, None]
                r.C3, r.C3_mag = b * rs, bmag * np.abs(rs)
            r.quad = np.stack([np.sum(acc * b, axis=(1, 2, 3)), np.sum(b * b, axis=(1, 2, 3))], axis=1)
            r.quad_mag = np.stack([np.sum(mag * bmag, axis=(1, 2, 3)), np.sum(bmag * bmag, axis=(1, 2, 3))], axis=1)
        r.n_terms = acc.shape[1] * acc.shape[2] * acc.shape[3]
    else:
        raise ValueError("no definition for epilogue %r" % (epi,))
    return r


# ------------------------------------------------------------------------------------------------ layouts
class Packed:
    """A logical (b2, b1, rows, cols) array laid out in a flat NaN-filled buffer: element (z2, z1, i, j) at
    base + z2 * s2 + z1 * s1 + i * ld + j; the buffer ends `guard` NaNs behind the furthest element.  flat[base:] is what a
    launch is given (base > 0: a column offset into wider rows, as production addresses D)."""

    def __init__(self, X, ld_pad=5, gap1=7, gap2=11, guard=64, base=0, share1=False, fill=np.nan):
        X = np.asarray(X, dtype=np.float64)
        b2, b1, rows, cols = X.shape
        self.ld = cols + ld_pad + base
        assert b1 == 1 or not share1
        self.s1 = 0 if share1 else rows * self.ld + gap1        # share1: one array for every inner entry (stride 0)
        self.s2 = max(b1 - 1, 0) * self.s1 + rows * self.ld + gap2
        self.base = base
        z2, z1, i, j = np.ix_(np.arange(b2), np.arange(b1), np.arange(rows), np.arange(cols))
        self.idx = base + z2 * self.s2 + z1 * self.s1 + i * self.ld + j
        self.flat = np.full(int(self.idx.max()) + 1 + guard, fill)
        self.flat[self.idx] = X
        self.inside = np.zeros(self.flat.size, dtype=bool)
        self.inside[self.idx] = True

    @property
    def given(self):
        return self.flat[self.base:]

    def take(self, flat_from_base):
        """The logical array out of a buffer of this layout (as returned by a launch: starting at base)."""
        return flat_from_base[self.idx - self.base]


def pack_vec(X, gap1=3, gap2=5, guard=16):
    """(b2, b1, n) or (b2, n) vectors -> flat NaN-padded buffer, strides (s1, s2)."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 2:
        X = X[:, None, :]
    p = Packed(X[:, :, None, :], ld_pad=0, gap1=gap1, gap2=gap2, guard=guard)
    return p


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
