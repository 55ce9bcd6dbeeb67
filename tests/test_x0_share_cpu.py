"""The shared-input sets of the executor (csrc/hrnet.hip: find_share_sets, mark_x0_share), host side, no GPU.

udp_debug_x0_share runs the pattern matcher alone over an op list and reports, per op, the op whose launch does its
work.  Checked here:

  * the planner's own programs: the mini HRNet that the GPU tests use (stage 2: fuse0 + one conv = 2 cout pairs;
    stage 3: fuse0 + two convs = 3 pairs; stage 4, a module with all four outputs: fuse0 + three convs = 4 pairs) and
    HRNet-W32 (one set per exchange unit that has an element-wise output 0: 7 sets, 8 + 7 carried ops);
  * the hazard decline: an op between two members that touches a member's output buffer, or writes one of its inputs,
    leaves that member out -- and the set disappears when fewer than two members remain;
  * two members that would run side by side while one writes what the other reads are not merged;
  * the limits: four cout pairs, three convs, one element-wise sum.
"""
import ctypes as C

from microprog import new_op
from udp_pose_amd import _lib, synth
from udp_pose_amd.hrnet_plan import HRNetProgram


def _sets(ops):
    arr = (_lib.ConvOp * len(ops))(*ops)
    carrier = (C.c_int * len(ops))()
    n = _lib.lib().udp_debug_x0_share(arr, len(ops), carrier)
    return n, list(carrier)


def _program_sets(extra, h, w):
    sd = synth.synth_state_dict(extra, 17, "gaussian", seed=3)
    prog = HRNetProgram(sd, extra, h, w, "f16x2")
    ops = list(prog.ops_array())
    n, carrier = _sets(ops)
    out = []
    for e in sorted(set(c for c in carrier if c >= 0)):
        members = [i for i, c in enumerate(carrier) if c == e]
        assert members[0] == e, "the launch sits at the earliest member"
        convs = [i for i in members if ops[i].kind == _lib.UDP_OP_CONV]
        fuse = [i for i in members if ops[i].kind == _lib.UDP_OP_FUSE]
        assert len(fuse) <= 1 and all(ops[i].ks == 3 and ops[i].stride == 2 and ops[i].cin == 32 for i in convs)
        assert len(set((ops[i].in_buf, ops[i].in_coff, ops[i].hin, ops[i].win) for i in members)) == 1
        out.append((sum(ops[i].cout_pad // 32 for i in convs), len(convs), len(fuse)))
    assert n == len(out)
    return out, prog


def test_mini_hrnet_forms_a_two_a_three_and_a_four_pair_set():
    extra = synth.scaled_extra(32, modules=(1, 1, 2), blocks=1)
    for h, w in ((64, 64), (96, 64)):
        sets, _ = _program_sets(extra, h, w)
        # stage 2, stage 3, the first module of stage 4; the last module has one output, a 1x1 conv: no set
        assert sets == [(2, 1, 1), (3, 2, 1), (4, 3, 1)], sets


def test_w32_forms_one_set_per_unit_with_an_elementwise_output():
    sets, prog = _program_sets(synth.W32_EXTRA, 256, 192)
    assert sets == [(2, 1, 1)] + [(3, 2, 1)] * 4 + [(4, 3, 1)] * 2, sets
    assert sum(c + f - 1 for _, c, f in sets) == 15          # launches saved: 7 fuse_sum + 8 stride-2 convs


def test_null_arguments():
    assert _lib.lib().udp_debug_x0_share(None, 1, (C.c_int * 1)()) == -1
    assert _lib.lib().udp_debug_x0_share((_lib.ConvOp * 1)(), 1, None) == -1


# ---------------------------------------------------------------- hand-made op lists
X0, UP, OUT0, R1, Y1, Y2, Y3, T = range(8)           # buffer ids


def _fuse(**kw):
    f = dict(cin=32, cout=32, hin=16, win=16, hout=16, wout=16, in_buf=X0, out_buf=OUT0, relu=1, n_up=1, up_buf=[UP], up_shift=[1])
    f.update(kw)
    return new_op(_lib.UDP_OP_FUSE, **f)


def _conv(cout, out_buf, **kw):
    f = dict(ks=3, stride=2, cin=32, cout=cout, hin=16, win=16, hout=8, wout=8, in_buf=X0, out_buf=out_buf, wfmt=1, relu=1, lane=1)
    f.update(kw)
    return new_op(_lib.UDP_OP_CONV, **f)


def _other(in_buf, out_buf, **kw):
    """An op that is no candidate: a 1x1 conv."""
    f = dict(cin=32, cout=32, hin=8, win=8, hout=8, wout=8, in_buf=in_buf, out_buf=out_buf, wfmt=1, lane=1)
    f.update(kw)
    return new_op(_lib.UDP_OP_CONV, **f)


def test_the_full_set_is_taken():
    ops = [_fuse(), _conv(64, Y1, res_buf=R1), _conv(32, Y2), _other(Y2, T), _conv(32, Y3)]
    assert _sets(ops) == (1, [0, 0, 0, -1, 0])
    # convs only (a last module: output 0 is a conv of its own)
    assert _sets(ops[1:]) == (1, [0, 0, -1, 0])
    # one conv and nothing else is no set
    assert _sets([_conv(64, Y1), _other(Y1, T)]) == (0, [-1, -1])


def test_an_op_between_that_touches_a_members_output_leaves_the_member_out():
    # the op between WRITES the buffer the last conv writes (the planner handed a dead tensor's buffer on) ...
    ops = [_fuse(), _conv(64, Y1), _other(Y1, Y3), _conv(32, Y3)]
    assert _sets(ops) == (1, [0, 0, -1, -1])
    # ... or READS it (its previous tenant is still live there)
    ops = [_fuse(), _conv(64, Y1), _other(Y3, T), _conv(32, Y3)]
    assert _sets(ops) == (1, [0, 0, -1, -1])
    # as an addend or a residual as well
    ops = [_fuse(), _conv(64, Y1), _other(Y1, T, n_up=1, up_buf=[Y3], up_shift=[1]), _conv(32, Y3)]
    assert _sets(ops) == (1, [0, 0, -1, -1])
    ops = [_fuse(), _conv(64, Y1), _other(Y1, T, res_buf=Y3), _conv(32, Y3)]
    assert _sets(ops) == (1, [0, 0, -1, -1])
    # control: the same list with the op between on buffers of its own
    ops = [_fuse(), _conv(64, Y1), _other(Y1, T), _conv(32, Y3)]
    assert _sets(ops) == (1, [0, 0, -1, 0])


def test_an_op_between_that_writes_a_members_input_leaves_the_member_out():
    # the residual of the conv is produced between the launch position and the conv
    ops = [_fuse(), _other(T, R1), _conv(64, Y1, res_buf=R1), _conv(32, Y2)]
    assert _sets(ops) == (1, [0, -1, -1, 0])
    # its up-sampled addend
    ops = [_fuse(), _other(T, R1), _conv(64, Y1, n_up=1, up_buf=[R1], up_shift=[1]), _conv(32, Y2)]
    assert _sets(ops) == (1, [0, -1, -1, 0])
    # fewer than two members remain: nothing changes
    ops = [_fuse(), _other(T, R1), _conv(64, Y1, res_buf=R1)]
    assert _sets(ops) == (0, [-1, -1, -1])
    # the shared view itself is rewritten: what follows reads another tensor
    ops = [_fuse(), _conv(64, Y1), _other(T, X0), _conv(32, Y2)]
    assert _sets(ops) == (1, [0, 0, -1, -1])


def test_members_that_would_race_inside_the_launch_are_not_merged():
    # the conv's output buffer is the addend the sum still reads (the planner frees it after the sum: same element count)
    ops = [_fuse(), _conv(64, Y1), _conv(32, UP)]
    assert _sets(ops) == (1, [0, 0, -1])
    # two convs into one buffer, and a conv whose residual is a sibling's output
    assert _sets([_fuse(), _conv(64, Y1), _conv(32, Y1)]) == (1, [0, 0, -1])
    assert _sets([_fuse(), _conv(32, Y2), _conv(64, Y1, res_buf=Y2)]) == (1, [0, 0, -1])
    # channel slices of one concat tensor: disjoint slices share no byte (the planner's programs: a conv writes
    # channels 0..31 of the tensor whose channels 32..95 a sibling reads as its residual); overlapping ones do,
    # and so do views with different pitches
    assert _sets([_conv(32, Y1, out_coff=0, out_pitch=64), _conv(32, Y1, out_coff=32, out_pitch=64)]) == (1, [0, 0])
    assert _sets([_fuse(), _conv(32, Y1, out_coff=0, out_pitch=96), _conv(64, Y2, res_buf=Y1, res_coff=32, res_pitch=96)]) == (1, [0, 0, 0])
    assert _sets([_conv(64, Y1, out_coff=0, out_pitch=96), _conv(32, Y1, out_coff=32, out_pitch=96)]) == (0, [-1, -1])
    assert _sets([_fuse(), _conv(32, Y1, out_coff=0, out_pitch=96), _conv(64, Y2, res_buf=Y1, res_coff=16, res_pitch=96)]) == (1, [0, 0, -1])
    assert _sets([_conv(32, Y1, out_coff=0, out_pitch=64), _conv(32, Y1, out_coff=32, out_pitch=96)]) == (0, [-1, -1])
    # an up-sampled addend is the whole buffer
    assert _sets([_fuse(), _conv(32, UP, out_coff=32, out_pitch=64)]) == (0, [-1, -1])


def test_a_wait_for_an_op_behind_the_launch_position_leaves_the_member_out():
    ops = [_fuse(), _conv(64, Y1), _other(T, R1, lane=2), _conv(32, Y2, n_wait=1, wait_op=[2])]
    assert _sets(ops) == (1, [0, 0, -1, -1])
    ops = [_other(T, R1, lane=2), _fuse(), _conv(64, Y1), _conv(32, Y2, n_wait=1, wait_op=[0])]
    assert _sets(ops) == (1, [-1, 1, 1, 1])


def test_limits_and_non_members():
    # four cout pairs: the third conv (64 channels) would make five -- left out, the next 32-channel one fits
    ops = [_fuse(), _conv(64, Y1), _conv(32, Y2), _conv(64, Y3), _conv(32, T)]
    assert _sets(ops) == (1, [0, 0, 0, -1, 0])
    # three convs
    ops = [_conv(32, Y1), _conv(32, Y2), _conv(32, Y3), _conv(32, T)]
    assert _sets(ops) == (1, [0, 0, 0, -1])
    # one element-wise sum
    ops = [_fuse(), _fuse(out_buf=T), _conv(64, Y1)]
    assert _sets(ops) == (1, [0, -1, 0])
    # not candidates: another view of the buffer, stride 1, 64 input channels, LDS-staged weights, a launch group,
    # a sum with a residual
    base = [_fuse(), _conv(64, Y1)]
    for bad in (_conv(32, Y2, in_coff=32, in_pitch=64), _conv(32, Y2, stride=1, hout=16, wout=16), _conv(32, Y2, cin=64),
                _conv(32, Y2, wfmt=0), _conv(32, Y2, group=3), _conv(32, Y2, in_buf=T)):
        assert _sets(base + [bad]) == (1, [0, 0, -1])
    assert _sets([_fuse(res_buf=R1), _conv(64, Y1), _conv(32, Y2)]) == (1, [-1, 1, 1])
