"""The exact text of every refusal of the six batch products that needs a live handle (tests/test_refusals_host.py has the NULL handle):
vors_batch_eval_pairs, _pose_information, _residual_maps, _reproject_depth, _fuse_depth, _point_cloud. GPU only.

One bad argument per call; status -1 and the whole message compared with ==. The expected strings are the library's own sentences, written
out here so that a changed sentence is noticed. Every output is a tensor filled with a sentinel that must still be there afterwards, and the
handle's workspace figure must not move: a refusal enqueues and allocates nothing. One good call per product at the end shows that the
default arguments of the table are good ones.

Handles: a dense and a candidate-list (coarse-to-fine) Batch of 2 pairs at 80x60 with 3 levels, each fresh (nothing prepared) and ready
(prepared and tracked), and one coarse-to-fine Trackers handle after one tracked frame for the sentences about a trackers-owned batch."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V

ROWS, COLS, L, N = 60, 80, 3, 2
INVALID = -1
SENTINEL = 0x5A
ABOVE_LIMIT = (1 << 20) + 4   # the first multiple of 4 above the stride limit of the batch products
OWNED = " is not available on a trackers-owned batch (the handle keeps records, not frames)"
INSPECTION = "keyframe inspection is not available on a trackers-owned batch in the candidate-list modes (the handle keeps records, not frames)"
EVAL_RANGE = "pair/level out of range (pair must be < the n_pairs of the last prepare_keyframes AND track_current)"


def stride_text(product, arg="model_stride_bytes"):
    return f"{product}: {arg} must be 0 or a multiple of 4 of at least 28"


def config(mode):
    intr = V.scaled_intrinsics(ROWS, COLS)
    return V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, arithmetic=V.ARITH_FUSED)


class Env:
    def __init__(self):
        import torch
        self.kg, self.kd, self.cg, self.cd, _ = V.synth_render_pairs(0x5EEDE7A9, N, ROWS, COLS, V.scaled_intrinsics(ROWS, COLS), want_cur_depth=True)
        self.models = torch.zeros((N + 1, 7), dtype=torch.float32, device="cuda")
        self.models[:, 6] = 1
        # every output of every product, as bytes: large enough for N + 1 pairs of the largest of them (residual_maps' warp field)
        self.outs = {name: torch.full(((N + 1) * ROWS * COLS * 8 + 8,), SENTINEL, dtype=torch.uint8, device="cuda") for name in "abcd"}
        self.zkey = torch.full(((N + 1) * ROWS * COLS + 1,), SENTINEL, dtype=torch.int64, device="cuda")
        self.fresh, self.ready = {}, {}
        for mode in (V.CANDIDATES_DENSE, V.CANDIDATES_COARSE_TO_FINE):
            self.fresh[mode] = V.Batch(config(mode), N, ROWS, COLS)
            b = self.ready[mode] = V.Batch(config(mode), N, ROWS, COLS)
            self.poses, self.status = torch.zeros((N, 7), dtype=torch.float32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
            b.track_pairs(self.kg, self.kd, self.cg, self.poses, self.status)
        self.trackers = V.Trackers(config(V.CANDIDATES_COARSE_TO_FINE), N, ROWS, COLS)
        self.trackers.init(self.kg, self.kd)
        self.trackers.track(self.cg, self.cd)
        torch.cuda.synchronize()
        # the batch handle of the sequences: the first member of vors_trackers (trackers.cpp); the C ABI has no accessor for it
        self.owned = C.c_void_p(C.cast(self.trackers._h, C.POINTER(C.c_void_p))[0])

    def handle(self, state, mode):
        return self.owned if state == "owned" else (self.fresh if state == "fresh" else self.ready)[mode]._h

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in self.outs.values()) and bool((self.zkey == SENTINEL).all())


@pytest.fixture(scope="module")
def env():
    return Env()


def ptr(t, offset=0):
    return None if t is None else C.c_void_p(t.data_ptr() + offset)


STREAM = V.Batch._stream


# Each product: the C call with good defaults (o overrides one of them) ...
def eval_pairs(e, h, **o):
    a = dict(n=N, level=0, k=1, models=ptr(e.models), stride=0, arith=V.ARITH_FUSED, what=0, sums=ptr(e.outs["a"]))
    a.update(o)
    return V.lib().vors_batch_eval_pairs(h, a["n"], a["level"], a["k"], a["models"], a["stride"], a["arith"], a["what"], a["sums"], STREAM())


def pose_information(e, h, **o):
    a = dict(n=N, level=0, models=ptr(e.models), stride=0, info=ptr(e.outs["a"]), cov=ptr(e.outs["b"]), sigma2=ptr(e.outs["c"]), flags=ptr(e.outs["d"]))
    a.update(o)
    return V.lib().vors_batch_pose_information(h, a["n"], a["level"], a["models"], a["stride"], a["info"], a["cov"], a["sigma2"], a["flags"], STREAM())


def residual_maps(e, h, **o):
    a = dict(n=N, level=0, models=ptr(e.models), stride=0, res=ptr(e.outs["a"]), uv=ptr(e.outs["b"]), hist=ptr(e.outs["c"]), scale=ptr(e.outs["d"]))
    a.update(o)
    return V.lib().vors_batch_residual_maps(h, a["n"], a["level"], a["models"], a["stride"], a["res"], a["uv"], a["hist"], a["scale"], STREAM())


def reproject_depth(e, h, **o):
    a = dict(n=N, level=0, models=ptr(e.models), stride=0, cur=ptr(e.cd), tol=0.01, z=ptr(e.outs["a"]), d=ptr(e.outs["b"]), res=ptr(e.outs["c"]),
             cnt=ptr(e.outs["d"]))
    a.update(o)
    return V.lib().vors_batch_reproject_depth(h, a["n"], a["level"], a["models"], a["stride"], a["cur"], a["tol"], a["z"], a["d"], a["res"], a["cnt"],
                                              STREAM())


def fuse_depth(e, h, **o):
    a = dict(n=N, models=ptr(e.models), stride=0, cur=ptr(e.cd), tol=0.01, kw=None, maxw=255, fill=0, zkey=ptr(e.zkey), d=ptr(e.outs["a"]),
             w=ptr(e.outs["b"]), cnt=ptr(e.outs["c"]))
    a.update(o)
    return V.lib().vors_batch_fuse_depth(h, a["n"], a["models"], a["stride"], a["cur"], a["tol"], a["kw"], a["maxw"], a["fill"], a["zkey"], a["d"],
                                         a["w"], a["cnt"], STREAM())


def point_cloud(e, h, **o):
    a = dict(n=N, level=0, poses=ptr(e.models), stride=0, keep=None, cap=ROWS * COLS, xyz=ptr(e.outs["a"]), pix=ptr(e.outs["b"]), gray=ptr(e.outs["c"]),
             cnt=ptr(e.outs["d"]))
    a.update(o)
    return V.lib().vors_batch_point_cloud(h, a["n"], a["level"], a["poses"], a["stride"], a["keep"], a["cap"], a["xyz"], a["pix"], a["gray"], a["cnt"],
                                          STREAM())


# ... and its refusals: (state of the handle, the one bad argument, the message). `lambda e:` where the argument needs the environment.
def strides(product, arg="model_stride_bytes"):
    return [("ready", dict(stride=s), stride_text(product, arg)) for s in (24, 30, ABOVE_LIMIT)]


def eval_state():
    """What check_eval refuses for the three products that read the current frame."""
    return [("fresh", {}, EVAL_RANGE), ("ready", dict(n=N + 1), EVAL_RANGE), ("ready", dict(level=-1), EVAL_RANGE), ("ready", dict(level=L), EVAL_RANGE),
            ("owned", {}, INSPECTION)]


def keyframe_state(product, level=True):
    """What the products of the keyframe side alone refuse."""
    n_pairs = f"{product}: n_pairs must be >= 1 and at most the n_pairs of the last prepare_keyframes"
    out = [("fresh", {}, f"{product} needs prepare_keyframes first"), ("owned", {}, product + OWNED), ("ready", dict(n=0), n_pairs),
           ("ready", dict(n=N + 1), n_pairs)]
    if level:
        out += [("ready", dict(level=-1), f"{product}: level out of range"), ("ready", dict(level=L), f"{product}: level out of range")]
    return out


NONE4 = "every output ({}) is NULL"
PRODUCTS = {
    "eval_pairs": (eval_pairs, [
        ("ready", dict(models=None), "eval_pairs: d_models is NULL"),
        ("ready", dict(sums=None), "eval_pairs: d_sums29 is NULL"),
        ("ready", dict(n=0), "eval_pairs: n_pairs must be >= 1"),
        ("ready", dict(k=0), "eval_pairs: models_per_pair must be >= 1"),
        ("ready", dict(k=1 << 26), "eval_pairs: n_pairs * models_per_pair is too large"),
        ("ready", dict(what=2), "eval_pairs: unknown `what` (VORS_EVAL_FULL or VORS_EVAL_ENERGY)"),
        ("ready", dict(arith=7), "unknown arithmetic mode"),
    ] + strides("eval_pairs") + eval_state()),
    "pose_information": (pose_information, [
        ("ready", dict(models=None), "pose_information: d_models is NULL"),
        ("ready", dict(n=0), "pose_information: n_pairs must be >= 1"),
    ] + strides("pose_information") + eval_state()),
    "residual_maps": (residual_maps, [
        ("ready", dict(models=None), "residual_maps: d_models is NULL"),
        ("ready", dict(res=None, uv=None, hist=None, scale=None), "residual_maps: " + NONE4.format("d_residuals, d_warp_uv, d_hist, d_scale")),
        ("ready", dict(hist=None), "residual_maps: d_scale needs d_hist (the pass keeps no histogram of its own)"),
        ("ready", dict(n=0), "residual_maps: n_pairs must be >= 1"),
    ] + strides("residual_maps") + eval_state()),
    "reproject_depth": (reproject_depth, [
        ("ready", dict(models=None), "reproject_depth: d_models is NULL"),
        ("ready", dict(z=None, d=None, res=None, cnt=None), "reproject_depth: " + NONE4.format("d_pred_z, d_pred_depth, d_depth_residual, d_counts")),
        ("ready", dict(z=None), "reproject_depth: d_pred_depth needs d_pred_z (the pass keeps no plane of its own)"),
        ("ready", dict(cur=None), "reproject_depth: d_depth_residual needs d_cur_depth"),
        ("ready", dict(level=1), "reproject_depth: d_cur_depth needs level 0 (depth maps exist at full resolution only)"),
        ("ready", dict(tol=float("nan")), "reproject_depth: tol_m must be >= 0 (and not NaN)"),
        ("ready", dict(tol=-1e-3), "reproject_depth: tol_m must be >= 0 (and not NaN)"),
        # (the level range needs a call without the current depth, which only level 0 may carry)
        ("ready", dict(level=-1, cur=None, res=None), "reproject_depth: level out of range"),
        ("ready", dict(level=L, cur=None, res=None), "reproject_depth: level out of range"),
    ] + strides("reproject_depth") + keyframe_state("reproject_depth", level=False)),
    "fuse_depth": (fuse_depth, [
        ("ready", dict(models=None), "fuse_depth: d_models is NULL"),
        ("ready", dict(cur=None), "fuse_depth: d_cur_depth is NULL"),
        ("ready", dict(zkey=None), "fuse_depth: d_zkey is NULL (the pass keeps no plane of its own)"),
        ("ready", lambda e: dict(zkey=ptr(e.zkey, 4)), "fuse_depth: d_zkey must be 8-byte aligned"),
        ("ready", dict(tol=float("nan")), "fuse_depth: tol_m must be >= 0 (and not NaN)"),
        ("ready", dict(tol=-1e-3), "fuse_depth: tol_m must be >= 0 (and not NaN)"),
        ("ready", dict(maxw=0), "fuse_depth: max_weight must be in 1..255"),
        ("ready", dict(maxw=256), "fuse_depth: max_weight must be in 1..255"),
        ("ready", dict(fill=-1), "fuse_depth: fill_min_weight must be in 0..255"),
        ("ready", dict(fill=256), "fuse_depth: fill_min_weight must be in 0..255"),
    ] + strides("fuse_depth") + keyframe_state("fuse_depth", level=False)),
    "point_cloud": (point_cloud, [
        ("ready", dict(xyz=None, pix=None, gray=None, cnt=None), "point_cloud: " + NONE4.format("d_xyz, d_pixel, d_gray, d_counts")),
        ("ready", dict(cap=-1), "point_cloud: negative capacity"),
        ("ready", dict(cap=0), "point_cloud: d_xyz / d_pixel / d_gray need capacity > 0"),
    ] + strides("point_cloud", "pose_stride_bytes") + keyframe_state("point_cloud")),
}


@pytest.mark.parametrize("mode", [V.CANDIDATES_DENSE, V.CANDIDATES_COARSE_TO_FINE], ids=["dense", "c2f"])
@pytest.mark.parametrize("product", list(PRODUCTS))
def test_refusals_in_these_words_and_nothing_enqueued(env, product, mode):
    call, cases = PRODUCTS[product]
    lib = V.lib()
    before = {state: env.fresh[mode].workspace_bytes() if state == "fresh" else env.ready[mode].workspace_bytes() for state in ("fresh", "ready")}
    owned_before = env.trackers.workspace_bytes()
    for state, bad, text in cases:
        bad = bad(env) if callable(bad) else bad
        st = call(env, env.handle(state, mode), **bad)
        said = lib.vors_last_error().decode()
        print(f"{product} [{state}] {bad}: {st} {said!r}")
        assert st == INVALID and said == text, (product, state, bad, st, said)
    assert env.untouched(), product
    assert env.fresh[mode].workspace_bytes() == before["fresh"] and env.ready[mode].workspace_bytes() == before["ready"]
    assert env.trackers.workspace_bytes() == owned_before


def test_the_default_arguments_are_good_ones(env):
    """The positive control of every product's table, on the dense and the candidate-list handle (kept last: these calls do write)."""
    import torch
    for mode, b in env.ready.items():
        for product, (call, _) in PRODUCTS.items():
            assert call(env, b._h) == 0, (product, mode, V.lib().vors_last_error().decode())
        torch.cuda.synchronize()
        assert not env.untouched()
