"""The case table of the weight-gradient arm tests (test_train_arms_cpu.py, test_gpu_train_arms.py).

udp_conv2d_wgrad (csrc/train.hip) has three kernel families, each instantiated for ks 1 and 3 and run at stride 1 and 2:

  * "f32"      wgrad_kernel<float, KS>    fp32 tensors, MFMA 16x16x4 fp32
  * "bf16"     wgrad_bf16_kernel<KS>      bf16 tensors, MFMA 32x32x16 bf16 behind transposed LDS reads
  * "bf16f32"  wgrad_kernel<__bf16, KS>   bf16 tensors on the fp32 MFMA kernel (UDP_POSE_WGRAD_F32MFMA, read per call)

A row names one call: the conv, the channel pitches of x and dy, the workspace as a number of partials (None: the size
udp_conv2d_wgrad_workspace_bytes suggests) and the accumulate flag.  ``plan(row, fam)`` asks the library's host-only
diagnostic udp_debug_wgrad_tile -- the function the launch path itself calls -- what geometry the call gets, and
``props(row, fam)`` turns that into the set of kernel branches the row executes.  Nothing here needs a GPU.

h and w are the INPUT map.  No map has more than 133 columns, no batch more than 4 images.
"""
import collections
import contextlib
import ctypes as C
import os

from udp_pose_amd import _lib

FAMILIES = ("f32", "bf16", "bf16f32")
FAMILY_CODE = {"f32": 0, "bf16": 1, "bf16f32": 2}
CELLS = [(f, ks, s) for f in FAMILIES for ks in (1, 3) for s in (1, 2)]
KNOB = "UDP_POSE_WGRAD_F32MFMA"

Row = collections.namedtuple("Row", "id ks stride cin cout h w n cin_k cout_k partials accumulate fams")
Plan = collections.namedtuple("Plan", "family tw th units_x units_y units upw splits pxp rows lds")


def _rup(x, m):
    return (x + m - 1) // m * m


def _row(ks, stride, cin, cout, h, w, n, cin_k=None, cout_k=None, partials=None, accumulate=0, fams=FAMILIES, tag=""):
    cin_k, cout_k = cin_k or _rup(cin, 16), cout_k or _rup(cout, 16)
    rid = "k%ds%d-%dto%d-%dx%dx%d" % (ks, stride, cin, cout, n, h, w)
    if (cin_k, cout_k) != (_rup(cin, 16), _rup(cout, 16)):
        rid += "-p%d.%d" % (cin_k, cout_k)
    if partials is not None:
        rid += "-ws%d" % partials
    if accumulate:
        rid += "-acc"
    return Row(rid + tag, ks, stride, cin, cout, h, w, n, cin_k, cout_k, partials, accumulate, tuple(fams))


ROWS = [
    # ragged last column unit (TW * units_x != wout), padded pixels, one image
    _row(3, 1, 16, 16, 5, 65, 1),
    _row(3, 2, 16, 16, 9, 65, 1),
    _row(1, 1, 16, 16, 5, 65, 1),
    _row(1, 2, 16, 16, 9, 131, 1),
    # ragged + pitches that are multiples of 8 but not of 16 (20 in 24, 36 in 40)
    _row(3, 1, 20, 36, 3, 67, 2, cin_k=24, cout_k=40),
    _row(1, 2, 20, 36, 5, 133, 2, cin_k=24, cout_k=40),
    # pitches that are multiples of 4 only: the fp32 kernel's ABI (bf16 tensors on it as well)
    _row(3, 2, 20, 12, 7, 9, 2, cin_k=20, cout_k=12, fams=("f32", "bf16f32")),
    _row(1, 1, 20, 12, 7, 9, 2, cin_k=20, cout_k=12, fams=("f32", "bf16f32")),
    # the bf16 kernel's stride-2 ragged row (wout 67), two images
    _row(3, 2, 16, 16, 3, 133, 2),
    _row(3, 2, 32, 32, 3, 133, 1),
    # odd input under stride 2 (7 -> 4, 9 -> 5), second cout tile half empty
    _row(1, 2, 32, 48, 7, 9, 3),
    _row(3, 2, 48, 32, 7, 9, 3),
    # second cin tile half empty; 17 couts in a pitch of 32; 9 * 17 * 48 is a multiple of 4, 9 * 17 * 3 below is not
    _row(3, 1, 48, 17, 7, 5, 3, cout_k=32),
    _row(3, 1, 3, 17, 7, 5, 3, cout_k=32),
    _row(1, 1, 3, 17, 7, 5, 3, cout_k=32),
    _row(1, 2, 17, 3, 7, 5, 2, cin_k=32),
    _row(3, 2, 17, 3, 7, 5, 2, cin_k=32),
    # one pixel
    _row(1, 1, 16, 16, 1, 1, 1),
    _row(3, 1, 16, 16, 1, 1, 2),
    _row(3, 2, 16, 16, 2, 2, 1),
    _row(1, 2, 16, 16, 1, 1, 2),
    # TH 13 / PX 143 in the bf16 kernel
    _row(1, 1, 64, 64, 13, 11, 3),
    # many units: the default workspace gives upw 1, a workspace of k partials a unit loop with a shorter last workgroup
    _row(3, 1, 32, 32, 11, 23, 2),
    _row(3, 1, 32, 32, 11, 23, 2, partials=4, accumulate=1),
    _row(3, 1, 32, 32, 11, 23, 2, partials=1),
    _row(3, 1, 16, 16, 5, 65, 4, partials=3),
    _row(3, 2, 16, 16, 9, 65, 4, partials=3, accumulate=1),
    _row(1, 1, 16, 16, 5, 65, 4, partials=3, accumulate=1),
    _row(1, 2, 16, 16, 9, 131, 4, partials=3),
    _row(1, 1, 32, 32, 11, 23, 2, partials=4),
    _row(1, 2, 32, 32, 21, 45, 2, partials=4, accumulate=1),
    _row(3, 2, 32, 32, 21, 45, 2, partials=4),
    # more than 16 partials: the second trip of the reduce's lane loop
    _row(3, 1, 16, 16, 24, 16, 4),
    _row(1, 1, 16, 16, 24, 16, 4, accumulate=1),
    _row(3, 2, 16, 16, 48, 32, 4),
    _row(1, 2, 16, 16, 48, 32, 4),
    _row(3, 1, 16, 16, 7, 130, 4, fams=("bf16",)),      # 84 units of one row each: no th in 2..5 divides 7
    _row(1, 1, 16, 16, 7, 130, 4, fams=("bf16",)),
    _row(1, 2, 16, 16, 9, 131, 4, fams=("bf16",), tag="-full"),
    # TH 1 by fallback under the fp32 kernel's stride-2 budget of 32 pixels (hout 3, wout 16: 2 does not divide 3)
    _row(1, 2, 16, 16, 5, 31, 1),
    _row(3, 2, 16, 16, 5, 31, 1),
    # the remaining (ks, stride) cells of the odd pitches and of the half-empty second tile
    _row(1, 1, 48, 17, 7, 5, 3, cout_k=32),
    _row(1, 1, 20, 36, 3, 67, 2, cin_k=24, cout_k=40),
    _row(3, 2, 20, 36, 5, 133, 2, cin_k=24, cout_k=40),
    # stride 2, ragged, EVEN width: the input column under the first missing output column (2 * wout - 1) is inside
    # the map, so a dy column staged past wout would meet real x.  With the odd widths above it meets staged zeros:
    # a hand-made mutant that ignored `ox < p.Wout` passed every stride-2 row until these were added
    _row(3, 2, 16, 16, 4, 130, 2),
    _row(3, 2, 16, 16, 4, 66, 1, fams=("f32", "bf16f32")),
]


@contextlib.contextmanager
def family_env(fam):
    """UDP_POSE_WGRAD_F32MFMA set for "bf16f32", unset otherwise; restored afterwards."""
    saved = os.environ.get(KNOB)
    try:
        os.environ.pop(KNOB, None)
        if fam == "bf16f32":
            os.environ[KNOB] = "1"
        yield
    finally:
        os.environ.pop(KNOB, None)
        if saved is not None:
            os.environ[KNOB] = saved


def dtype_of(fam):
    return "f32" if fam == "f32" else "bf16"


def out_hw(row):
    pad = row.ks // 2
    return (row.h + 2 * pad - row.ks) // row.stride + 1, (row.w + 2 * pad - row.ks) // row.stride + 1


def per_bytes(row):
    return row.ks * row.ks * row.cout * row.cin * 4


def workspace_bytes(row):
    if row.partials is None:
        return int(_lib.lib().udp_conv2d_wgrad_workspace_bytes(row.cout, row.cin, row.ks))
    return row.partials * per_bytes(row)


def debug_tile(fam, n, h, w, cin_k, ho, wo, cout_k, ks, stride, cout, cin, ws_bytes):
    """(return code, Plan or None) of udp_debug_wgrad_tile in the family's environment."""
    out = (C.c_int * 11)()
    with family_env(fam):
        rc = _lib.lib().udp_debug_wgrad_tile(n, h, w, cin_k, ho, wo, cout_k, ks, stride, cout, cin,
                                             _lib.DTYPES[dtype_of(fam)], ws_bytes, out)
    return rc, (Plan(*out) if rc == 0 else None)


def plan(row, fam):
    ho, wo = out_hw(row)
    rc, p = debug_tile(fam, row.n, row.h, row.w, row.cin_k, ho, wo, row.cout_k, row.ks, row.stride, row.cout, row.cin,
                       workspace_bytes(row))
    assert rc == 0, "%s / %s: udp_debug_wgrad_tile refused it (%d: %s)" % (row.id, fam, rc, _lib.lib().udp_last_error())
    assert p.family == FAMILY_CODE[fam]
    return p


def max_px(fam, stride):
    """The pixel budget of a unit (csrc/train.hip, wgrad_plan): what TH could have been if the map's height allowed."""
    return 256 if fam == "bf16" else (64 if stride == 1 else 32)


PROPS = ("ragged", "ragged_seen", "th1_fallback", "th_gt1", "px_padded", "px1", "upw3_short_last", "upw1", "splits_2_15", "splits_gt16",
         "per_not_x4", "chan_not_x32", "second_tile_partial", "pitch_not_x16", "odd_input_s2", "accumulate", "n1")


def props(row, fam):
    """The branches of the kernels this row executes in this family, from the diagnostic's report."""
    p = plan(row, fam)
    ho, wo = out_hw(row)
    px = p.th * p.tw
    got = set()
    if p.tw * p.units_x != wo:
        got.add("ragged")                                  # `ox < p.Wout` runs false
        # ... and the result depends on it: tap kx = 0 of the first missing column wo reads input column
        # wo * stride - pad, which is inside the map (a 1x1 conv reads wo * stride >= w there: staged zeros)
        if row.ks == 3 and wo * row.stride - 1 < row.w:
            got.add("ragged_seen")
    if p.th == 1 and ho > 1 and 2 * p.tw <= max_px(fam, row.stride):
        got.add("th1_fallback")                            # the budget allowed rows, no th divided hout / fitted
    if p.th > 1:
        got.add("th_gt1")
    if px != p.pxp:
        got.add("px_padded")                               # PX % 4 (16) != 0: zero rows PX..PXP, the min(q, PX - 1) clamp
    if px == 1:
        got.add("px1")
    if p.upw >= 3 and p.units % p.upw:
        got.add("upw3_short_last")                         # unit loop, its leading barrier, prefetch; u1 = units cuts
    if p.upw == 1:
        got.add("upw1")
    if 2 <= p.splits <= 15:
        got.add("splits_2_15")
    if p.splits > 16:
        got.add("splits_gt16")                             # the reduce's `k += 16` lane loop takes a second trip
    if (row.ks * row.ks * row.cout * row.cin) % 4:
        got.add("per_not_x4")                              # the reduce's scalar tail
    if row.cin % 32 or row.cout % 32:
        got.add("chan_not_x32")
    if (row.cin > 32 and row.cin % 32) or (row.cout > 32 and row.cout % 32):
        got.add("second_tile_partial")
    if row.cin_k % 16 or row.cout_k % 16:
        got.add("pitch_not_x16")                           # `c0 + c4 < pitch` cuts inside a 16-channel half
    if row.stride == 2 and (row.h % 2 or row.w % 2):
        got.add("odd_input_s2")
    if row.accumulate:
        got.add("accumulate")
    if row.n == 1:
        got.add("n1")
    return got


def cases():
    """(row, family) pairs of the GPU test."""
    return [(r, f) for r in ROWS for f in FAMILIES if f in r.fams]
