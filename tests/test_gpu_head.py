"""GPU: the four C-ABI calls of the training head -- hipac_linear_forward / hipac_linear_backward,
hipac_cross_entropy_fwd_bwd, hipac_adam_step, hipac_ntxent_fwd_bwd (csrc/train.hip, csrc/ntxent.hip) -- against float64
references (tests/head_cpu.py) on the cases of tests/head_cases.py: the shapes at the kernels' own tile, group and grid
boundaries, never the workload's size.  The calls go through capi.load_library() with raw pointers: NativeLinear and
FlatAdam cannot express guard bands, a NULL dx or a start from non-zero optimizer state.

Gates (tests/head_cases.py).  Linear outputs (y, dx, dw, db): element-wise and derived,
|got - ref64| <= (L + 3) * 2^-24 * S with L the reduction length and S the float64 sum of |products| (+ |bias|,
+ |previous value| when accumulating); S = 0 means exact; the ReLU-masked dy is compared bitwise.  Cross-entropy, Adam,
NT-Xent: 10 x the distance the float32 stand-in (plain torch float32 on the CPU) keeps from the float64 reference on
these inputs, metric max|a - b| / max|b| (Adam's p: on the move p_new - p_old), the largest figure of a (primitive,
tensor, input kind) group; measured by tests/tools/measure_head_fp32.py into tests/golden/head_fp32_distances.json, never
against the native code.  tests/test_oracle_head.py shows on the CPU that each gate can fail: a stand-in with one injected
fault at a time (dropped K tail, y >= 0 mask, overwritten accumulate, lost row / column / element tails, eps inside the
square root, ...) is caught by the case built for it.

Guards.  Every native output buffer (y, dym, dx, dw, db, loss, dlogits, both scratches, dz, p, m, v) is followed by 64
floats of a sentinel bit pattern that must survive the call, and starts out filled with it (a NaN), so an element the
kernel does not write shows; every input buffer is followed by 64 NaNs (labels: 64 out-of-range labels), so a read
past the end shows in a result.

Two gates say little, by construction: ntxent.loss.zj_eq_zi (with z_j == z_i at t = 0.05 the loss is 1e-8 left over from
terms of 20; float32 itself is 100 % off) and adam.move.* for parameters of magnitude 1 (the move of 1e-3 sits on p's own
rounding of 6e-8: 1.6e-4); the small_p and x1e-12 kinds are there for the latter, dz for the former.

The native figures on an MI355X (largest of each group / its gate; every test prints its own before it asserts).
Linear, worst |got - ref64| / bound per shape: (1,1,1) 0.170, (1,2,31) 0.247, (63,65,32) 0.072, (64,64,33) 0.073,
(65,63,64) 0.057, (129,1,95) 0.248, (2,130,1) 0.354, (15,17,70) 0.147, (16,128,512) 0.187 (dw; its forward, K = 512: 0.006);
every masked dy bitwise right.  Where the reduction is short the MFMA's in-order fused sum lands on the very bits of the
CPU's, so several of these equal the stand-in's own ratios.
    ce      loss: randn 1.1e-7 / 1.3e-6, spread1e4 1.6e-7 / 1.0e-6, equal_block 1.3e-7 / 8.2e-7
            dlogits: randn 1.6e-7 / 1.9e-6, spread1e4 9.2e-8 / 1.0e-6, equal_block 1.5e-7 / 1.6e-6
    adam    move: randn 1.6e-4 / 1.6e-3, x1e4 3.6e-4 / 3.6e-3, x1e-12 5.9e-5 / 5.9e-4, zeros 1.8e-4 / 1.8e-3,
            small_p 1.3e-7 / 1.1e-6;  m: 8.0e-8 .. 1.3e-7 / 8.0e-7 .. 1.3e-6;  v: 8.8e-8 .. 1.4e-7 / 8.8e-7 .. 1.4e-6
            (element-wise IEEE operations: m, v and most moves come out at the stand-in's own distance); zero places exact
    ntxent  loss: plain 3.8e-7 / 1.9e-6, x1e-3 6.9e-8 / 7.8e-7, x1e3 7.4e-8 / 2.1e-6, identical 9.6e-8 / 1.6e-6,
            zero_row 2.9e-8 / 2.9e-7, zj_eq_zi 1.0 / 10 (see above; 3.5e-7 at n = 129)
            dz: plain 6.1e-7 / 7.1e-6, x1e-3 5.4e-7 / 5.5e-6, x1e3 5.9e-7 / 5.8e-6, identical 8.0e-7 / 7.1e-6,
            zj_eq_zi 2.0e-6 / 2.3e-5, zero row 3.4e-7 / 4.1e-6, the rows beside it 1.0e-6 / 1.1e-5
No guard band was touched, and every repeated call gave the same bits.
"""
import numpy as np
import pytest
import torch

import head_cases as cases
import head_cpu as H
from ss25_hierarchical_multiscale_image_classification_amd import capi

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x7FC5A3E1  # a quiet NaN with a recognisable payload


class Native:
    """The C ABI on guarded device buffers; numpy in, numpy out (the interface of head_cpu.StandIn)."""

    def __init__(self):
        self.lib = capi.load_library()
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self.outs = []

    def out(self, name, n, init=None):
        buf = torch.empty(n + GUARD, dtype=torch.float32, device=self.dev)
        buf.view(torch.int32).fill_(SENTINEL)
        if init is not None:
            buf[:n].copy_(torch.from_numpy(np.array(init, dtype=np.float32).ravel()))
        self.outs.append((name, buf, n))
        return buf

    def inp(self, a):
        a = np.array(a, dtype=np.float32).ravel()
        buf = torch.full((a.size + GUARD,), float("nan"), dtype=torch.float32, device=self.dev)
        buf[: a.size].copy_(torch.from_numpy(a))
        return buf

    def call(self, what, rc):
        capi._check(rc, what)
        torch.cuda.synchronize()
        for name, buf, n in self.outs:
            tail = buf[n:].view(torch.int32).cpu()
            assert bool((tail == SENTINEL).all()), f"{what}: wrote behind {name} ({int((tail != SENTINEL).sum())} of {GUARD} guard floats)"
        self.outs = []

    @staticmethod
    def host(buf, *shape):
        n = int(np.prod(shape))
        return buf[:n].cpu().numpy().reshape(shape)

    def linear_forward(self, x, w, b, relu):
        (M, K), N = x.shape, w.shape[0]
        xd, wd, bd, y = self.inp(x), self.inp(w), self.inp(b), self.out("y", M * N)
        self.call("hipac_linear_forward", self.lib.hipac_linear_forward(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(),
                                                                        M, N, K, int(relu), capi._stream()))
        return self.host(y, M, N)

    def linear_backward(self, x, w, dy, y, dw0, db0, accumulate, want_dx):
        (M, K), N = x.shape, w.shape[0]
        xd, wd, gd = self.inp(x), self.inp(w), self.inp(dy)
        yd = None if y is None else self.inp(y)
        dym = None if y is None else self.out("dym", M * N)
        dx = self.out("dx", M * K) if want_dx else None
        # accumulate = 0 must overwrite: the buffers start as NaNs then
        dw = self.out("dw", N * K, dw0 if accumulate else None)
        db = self.out("db", N, db0 if accumulate else None)
        self.call("hipac_linear_backward", self.lib.hipac_linear_backward(
            xd.data_ptr(), wd.data_ptr(), gd.data_ptr(), capi._ptr(yd), capi._ptr(dym), capi._ptr(dx), dw.data_ptr(), db.data_ptr(),
            M, N, K, int(accumulate), capi._stream()))
        return (None if dym is None else self.host(dym, M, N), None if dx is None else self.host(dx, M, K),
                self.host(dw, N, K), self.host(db, N))

    def cross_entropy(self, logits, labels, class_w):
        M, C = logits.shape
        ld = self.inp(logits)
        lab = torch.full((M + GUARD,), -1, dtype=torch.int64, device=self.dev)
        lab[:M].copy_(torch.from_numpy(np.array(labels, dtype=np.int64)))
        cwd = None if class_w is None else self.inp(class_w)
        loss, dl = self.out("loss", 1), self.out("dlogits", M * C)
        scratch = self.out("scratch", 2 + 8 * ((M + 255) // 256))  # the size the header promises to stay inside
        self.call("hipac_cross_entropy_fwd_bwd", self.lib.hipac_cross_entropy_fwd_bwd(
            ld.data_ptr(), lab.data_ptr(), capi._ptr(cwd), M, C, loss.data_ptr(), dl.data_ptr(), scratch.data_ptr(), capi._stream()))
        return self.host(loss, 1)[0], self.host(dl, M, C)

    def adam_steps(self, p, grads, m, v, step, lr, beta1, beta2, eps):
        n = p.size
        pd, md, vd = self.out("p", n, p), self.out("m", n, m), self.out("v", n, v)
        guarded = list(self.outs)
        for k, g in enumerate(grads):
            gd = self.inp(g)
            self.outs = list(guarded)  # the guards are checked after every step
            self.call("hipac_adam_step", self.lib.hipac_adam_step(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n,
                                                                  lr, beta1, beta2, eps, step + k, capi._stream()))
        return self.host(pd, n), self.host(md, n), self.host(vd, n)

    def ntxent(self, z, temperature, want_grad=True):
        rows, d = z.shape
        n = rows // 2
        nbytes = self.lib.hipac_ntxent_scratch_bytes(n, d)
        assert nbytes % 4 == 0
        zd, loss, scratch = self.inp(z), self.out("loss", 1), self.out("scratch", nbytes // 4)
        dz = self.out("dz", rows * d) if want_grad else None
        self.call("hipac_ntxent_fwd_bwd", self.lib.hipac_ntxent_fwd_bwd(zd.data_ptr(), n, d, float(temperature), loss.data_ptr(),
                                                                        capi._ptr(dz), scratch.data_ptr(), nbytes, capi._stream()))
        return self.host(loss, 1)[0], (None if dz is None else self.host(dz, rows, d))


@pytest.fixture(scope="module")
def native():
    return Native()


def assert_inside_gates(tag, figs):
    bad = cases.over_gate(tag, figs)
    assert not bad, (tag, bad)


@pytest.mark.parametrize("shape", cases.LINEAR_SHAPES, ids=str)
def test_linear_forward_and_backward_inside_the_float32_sum_bound(native, shape):
    """Forward with bias, with and without ReLU; backward with and without the mask, accumulate 0 and 1 (onto random dw / db),
    dx given and NULL; on (15, 17, 70) also the mask from a y that holds +0, -0, FLT_MIN, -FLT_MIN and NaN."""
    r = cases.linear_ratios(native, shape)
    k = max(r, key=r.get)
    print(f"[head] linear {shape}: worst bound ratio {r[k]:.3f} ({k}); " + ", ".join(f"{a} {b:.3f}" for a, b in r.items()))
    assert all(v <= 1.0 for v in r.values()), {a: b for a, b in r.items() if not b <= 1.0}


@pytest.mark.parametrize("case", cases.ce_case_list(), ids=lambda c: c[0])
def test_cross_entropy_matches_float64(native, case):
    assert_inside_gates(case[0], cases.ce_figures(native, case))


def test_cross_entropy_bad_labels_give_nan_and_weight_zero(native):
    """Labels -1, C and 2^40 in rows 0, 128 and 256 of a (257, 3) batch: a NaN loss, NaN gradient rows, and every other
    row as if the three were not in the batch (the kernel gives them weight 0)."""
    logits, labels, cw, good = cases.ce_bad_label_inputs()
    loss, dl = native.cross_entropy(logits, labels, cw)
    _, ref = H.cross_entropy(logits[good], labels[good], cw)
    assert np.isnan(loss)
    assert np.isnan(dl[list(cases.BAD_LABELS)]).all()
    assert_inside_gates("ce-bad-labels", {"ce.dlogits.randn": cases.rel(dl[good], ref)})


def test_cross_entropy_twice_gives_the_same_bits(native):
    logits, labels, cw = cases.ce_inputs((513, 5), "random", "randn")
    a, b = native.cross_entropy(logits, labels, cw), native.cross_entropy(logits, labels, cw)
    assert cases.same_bits(a[0], b[0]) and cases.same_bits(a[1], b[1])


@pytest.mark.parametrize("case", cases.adam_case_list(), ids=lambda c: c[0])
def test_adam_matches_float64(native, case):
    assert_inside_gates(case[0], cases.adam_figures(native, case))


@pytest.mark.parametrize("case", cases.ntxent_case_list(), ids=lambda c: c[0])
def test_ntxent_matches_float64_and_repeats_its_bits(native, case):
    z, t = cases.ntxent_inputs(case[1], case[2]), case[1][2]
    loss, dz = native.ntxent(z, t, True)
    assert_inside_gates(case[0], cases.ntxent_figures(native, case, got=(loss, dz)))
    loss2, dz2 = native.ntxent(z, t, True)  # "the loss is summed in row order": no atomics anywhere, the same bits
    assert cases.same_bits(loss, loss2) and cases.same_bits(dz, dz2)
    loss3, none = native.ntxent(z, t, False)
    assert none is None and cases.same_bits(loss, loss3)
