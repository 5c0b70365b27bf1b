"""How each DiscreteVAE convolution is lowered onto the GEMMs, stated once per layer and free of torch and of the library, so
that it can be checked on any machine (tests/test_vae_lowering.py).

A convolution is a set of TAP PRODUCTS: a [B*H*W, C] activation read through a tap list with a stride onto an output grid,
multiplied by one derived weight copy.  `_Conv` builds the products of its layer (forward, weight gradient, input gradient) when it
is made; models.py launches them (`_tap_product`, `_tap_wgrad`), and everything that restates the same geometry -- the layout of
the derived weight copies, the tables of the two batched refresh launches, the column scratch, the workspace bounds -- is derived
from the same records below.

  kind   forward                            weight gradient                         input gradient
  down   x, TAPS4, stride 2, wf             the forward's gather of x               4 parity products of dy, stride 1, wp[q]
  res    x, TAPS3, stride 1, wf             the forward's gather of x               dy, TAPS3_REV, wd
  up     4 parity products of x, wp[q]      gather of dz, TAPS4, stride 2, onto     the same gather, times wd
                                            (H, W); the bias is a column sum
  final  x itself (one-tap im2col when      x itself                                plain product against the kernel (no record)
         cin is no multiple of 64), wf
"""
import math
from collections import namedtuple

OUT_CP = 64    # padded reconstruction channels
ALIGN = 128    # every flat-buffer entry starts on a multiple of this many elements


def _ru(x, m):
    return (x + m - 1) // m * m


TAPS4 = [(ky - 1, kx - 1) for ky in range(4) for kx in range(4)]       # 4x4 s2 SAME: pad 1 before (Appendix A.8)
TAPS3 = [(ky - 1, kx - 1) for ky in range(3) for kx in range(3)]       # 3x3 s1 SAME
TAPS3_REV = [(1 - ky, 1 - kx) for ky in range(3) for kx in range(3)]   # input gradient of the 3x3 conv
TAP1 = [(0, 0)]


def _parity(p):
    """output-parity class of the stride-2 adjoint: [(k index, dy, dx)] for the 2x2 contributing taps."""
    def ax(par):
        return [(1, 0), (3, -1)] if par == 0 else [(0, 1), (2, 0)]   # (k, source offset)
    py, px = p >> 1, p & 1
    return [(ky * 4 + kx, dy, dx) for (ky, dy) in ax(py) for (kx, dx) in ax(px)]


def _p2(v):
    return v > 0 and (v & (v - 1)) == 0


def gemm_gathers(C):
    """dmi_conv_gemm_nt gathers the taps inside the product: it needs C % 64 == 0"""
    return C % 64 == 0


def wgrad_gathers(C, Ho, Wo):
    """dmi_conv_wgrad_tn gathers the taps inside the weight gradient: C % 64 == 0 and power-of-two output dims"""
    return gemm_gathers(C) and _p2(Ho) and _p2(Wo)


def implicit_ok(c):
    """down / res layers: forward and weight gradient read the same gather of x, so they go together -- both implicit, or the
    forward materialises its column and keeps it for the weight gradient (the input gradient decides for itself)"""
    return wgrad_gathers(c.cin, c.Ho, c.Wo)


# (H, W, C) source geometry, (Ho, Wo) output grid; K = len(taps) * C rows on the pitch Kp; N output columns; the product multiplies
# by the derived copy `copy` = ("wf", None) / ("wd", None) / ("wp", parity), which holds the kernel taps `kidx` (None: all of
# them, transposed); implicit: gathered inside the GEMM; direct: one tap on the pitch C -- the activation is its own column
Product = namedtuple("Product", "H W C Ho Wo stride taps K Kp N copy kidx implicit direct")


def _product(H, W, C, Ho, Wo, stride, taps, N, copy=None, kidx=None, implicit=False, direct=False):
    K = len(taps) * C
    return Product(H, W, C, Ho, Wo, stride, taps, K, K if direct else _ru(K, 64), N, copy, kidx, implicit, direct)


class _Conv:
    def __init__(self, name, kind, cin, cout, H, W, cin_ref=None, cout_ref=None):
        self.name, self.kind, self.cin, self.cout, self.H, self.W = name, kind, cin, cout, H, W
        self.cin_ref = cin if cin_ref is None else cin_ref     # channels of the reference variable
        self.cout_ref = cout if cout_ref is None else cout_ref
        self.kk = {"down": 16, "up": 16, "res": 9, "final": 1}[kind]
        Ho, Wo = self.Ho, self.Wo = {"down": (H // 2, W // 2), "up": (2 * H, 2 * W)}.get(kind, (H, W))
        # kernel stored [kk][A][Bn]: conv: A=cin, Bn=cout ; conv-transpose (TF [kh,kw,Cout,Cin]): A=cout(z), Bn=cin(y)
        self.A, self.Bn = (cout, cin) if kind == "up" else (cin, cout)
        # fwd, dgrad: tuples of products (four for the parity classes of a stride-2 adjoint, then a pixel interleave); wgrad: one
        if kind in ("down", "res"):
            taps, s = (TAPS4, 2) if kind == "down" else (TAPS3, 1)
            self.fwd = (_product(H, W, cin, Ho, Wo, s, taps, cout, ("wf", None), implicit=implicit_ok(self)),)
            self.wgrad = self.fwd[0]
            if kind == "res":
                self.dgrad = (_product(H, W, cout, H, W, 1, TAPS3_REV, cin, ("wd", None), list(range(9)), gemm_gathers(cout)),)
            else:
                self.dgrad = self._parity_products(Ho, Wo, cout, cin)
        elif kind == "up":
            self.fwd = self._parity_products(H, W, cin, cout)
            self.wgrad = _product(Ho, Wo, cout, H, W, 2, TAPS4, cin, ("wd", None), implicit=wgrad_gathers(cout, H, W))
            self.dgrad = (self.wgrad,)
        else:
            self.fwd = (_product(H, W, cin, H, W, 1, TAP1, cout, ("wf", None), direct=gemm_gathers(cin)),)   # (plain dmi_gemm_nt: K % 64 == 0)
            self.wgrad = _product(H, W, cin, H, W, 1, TAP1, cout, direct=True)
            self.dgrad = None

    @staticmethod
    def _parity_products(H, W, C, N):
        return tuple(_product(H, W, C, H, W, 1, [(t[1], t[2]) for t in _parity(q)], N, ("wp", q), [t[0] for t in _parity(q)],
                              gemm_gathers(C)) for q in range(4))

    def products(self):
        """the products that own a derived weight copy, in layout order"""
        return self.fwd + (self.dgrad or ())


def build_graph(Hs, img_cp, c_st, convblocks, n_hid, num_tokens):
    """the layer list of the encoder (n_enc of them) and the decoder, and the flat parameter layout: (convs, n_enc, offset, shape,
    total)"""
    convs, H, cin, cin_ref, n_enc = [], Hs, img_cp, c_st, None
    stages = [("encoder", "down", b, blk) for b, blk in enumerate(convblocks)] + \
             [("decoder", "up", b, blk) for b, blk in enumerate(reversed(convblocks))]
    for side, kind, b, (stack, ch) in stages:
        if (side, b) == ("decoder", 0):
            n_enc = len(convs)
        for i in range(stack):
            p = f"{side}/block_{b}/layer_{i}/"
            if i == 0:
                convs.append(_Conv(f"{p}conv_{kind}sample", kind, cin, ch, H, H, cin_ref=cin_ref))
                H = H // 2 if kind == "down" else H * 2
            else:
                convs += [_Conv(p + "conv_in", "res", ch, ch, H, H), _Conv(p + "conv_out", "res", ch, ch, H, H)]
        cin = cin_ref = ch
    convs.append(_Conv("decoder/conv2d", "final", cin, OUT_CP, H, H, cout_ref=c_st))
    offset, shape, off = {}, {}, 0
    for i, c in enumerate(convs):
        entries = [(c.name + "/kernel", (c.kk, c.A, c.Bn)), (c.name + "/bias", (c.cout,))]
        for name, shp in [("codebook/codebook", (n_hid, num_tokens))] * (i == n_enc) + entries:
            offset[name], shape[name] = off, shp
            off += _ru(math.prod(shp), ALIGN)
    return convs, n_enc, offset, shape, off


def weight_copies(convs, n_hid, num_tokens):
    """the derived weight copies as views of one flat buffer: ([(kind, name, q, rows, cols)], {(kind, name, q): offset}, size);
    every product's copy [N][Kp] in layer order, then the transposed codebook"""
    plan = [(t.copy[0], c.name, t.copy[1], t.N, t.Kp) for c in convs for t in c.products()]
    plan.append(("cb", "codebook_t", None, num_tokens, n_hid))
    off, offs = 0, {}
    for kind, name, q, rows, cols in plan:
        offs[(kind, name, q)] = off
        off += _ru(rows * cols, ALIGN)
    return plan, offs, off


def _tiles(R, C):
    return ((R + 63) // 64) * ((C + 63) // 64)


def refresh_tables(convs, offset, wc_off, n_hid, num_tokens):
    """rows of the two batched refresh launches: dmi_transpose_bf16_batch [src, dst, R, C, first tile] for the copies that hold
    the whole kernel transposed, dmi_weight_gather_batch [src, dst, A, Bn, n, ldo, first block, 16 tap indices] for those that hold
    some of its taps; a transpose whose rows need zero padding to the pitch keeps its own launch (`padded`)"""
    tr, tiles, ga, blocks, padded = [], 0, [], 0, []
    for c in convs:
        src = offset[c.name + "/kernel"]
        for t in c.products():
            kind, q = t.copy
            dst = wc_off[(kind, c.name, q)]
            if t.kidx is not None:
                ga.append([src, dst, c.A, c.Bn, len(t.kidx), t.Kp, blocks] + t.kidx + [0] * (16 - len(t.kidx)))
                blocks += (c.A * t.Kp + 2047) // 2048
            elif t.Kp == t.K:
                tr.append([src, dst, t.K, t.N, tiles])
                tiles += _tiles(t.K, t.N)
            else:
                padded.append((c.name, kind, t.K, t.Kp, t.N))
    tr.append([offset["codebook/codebook"], wc_off[("cb", "codebook_t", None)], n_hid, num_tokens, tiles])
    tiles += _tiles(n_hid, num_tokens)
    return dict(tr=tr, tiles=tiles, ga=ga, blocks=blocks, padded=padded)


def max_col(convs, B):
    """elements of the largest column matrix of any product (implicit ones included: the scratch keeps its size)"""
    return max(B * t.Ho * t.Wo * t.Kp for c in convs for t in c.products())


def wgrad_bounds(convs, B):
    """per layer (M, K, N) bounding its weight-gradient product and column sum either way round: what sizes ws, ws_cs, ws_pool"""
    return [(B * max(c.Ho * c.Wo, c.H * c.W), c.kk * max(c.cin, c.cout), max(c.cin, c.cout)) for c in convs]
