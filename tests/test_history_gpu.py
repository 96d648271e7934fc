"""The temporal history on the GPU (csrc/pt_history.h, include/ptgpu.h pt_history_*): k_hist_advance and everything around it
against tests/history_model.py, bit for bit; resolve and the film filter on the history's planes against film_model /
film_denoise_model; add_frame against the model fed with the planes of entry points that are tested already."""
import numpy as np
import pytest

import aov_model as am
import film_denoise_model as fdm
import history_model as hm

pytestmark = pytest.mark.gpu
f32 = np.float32
N = 4
PT_FLAG_MEGAKERNEL = 8
MAX = 1 << 24


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def hparams(pta, p):
    return pta.HistoryParams(p.normal_cos, p.plane_tol, p.max_samples, p.rotate)


PARAMS = hm.DEFAULTS._replace(max_samples=6)        # (the third frame of a chain meets the cap)
FRONT = hm.look_at((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), fov=0.9)
PLANES = [((0.0, 0.0, -1.5), (0.0, 0.0, 1.0), lambda P: (np.abs(P[:, 0]) < 0.25) & (P[:, 1] < 0.4)),
          ((0.0, 0.0, -4.0), (0.0, 0.0, 1.0), lambda P: P[:, 1] < 1.2),
          ((0.0, -0.8, 0.0), (0.0, 1.0, 0.0), lambda P: P[:, 2] > -4.0)]
CHAIN = (FRONT, hm.look_at((0.21, 0.03, 0.0), (0.23, 0.0, -1.0), fov=0.9), hm.look_at((0.4, 0.05, 0.1), (0.33, 0.02, -1.0), fov=0.9))


def synthetic_frames(w, h, cameras=CHAIN, planes=PLANES):
    out = []
    for k, cam in enumerate(cameras):
        a, m = hm.noise_planes(w * h, N, 100 * w + k)
        out.append((cam, a, m, hm.plane_records(cam, w, h, N, planes)))
    return out


def check_state(hist, want, aov, where):
    acc, mom, cnt, surf, guides = hist.read()
    assert same_bits(surf, want["surf"]), (where, "surf")
    assert np.array_equal(cnt, want["count"]), (where, "count")
    assert same_bits(acc, want["accum"]), (where, "accum", int((bits(acc) != bits(want["accum"])).any(axis=1).sum()))
    assert same_bits(mom, want["moments"]), (where, "moments")
    assert same_bits(guides, am.guides_of(aov, N)), (where, "guides")


@pytest.mark.parametrize("size", [(1, 1), (3, 2), (64, 4), (37, 23)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_three_chained_frames_equal_the_model_bit_for_bit(pta, size):
    w, h = size
    hist = pta.History(w, h, hparams(pta, PARAMS))
    model, vprev = None, None
    seen, taps = set(), set()
    for k, (cam, a, m, aov) in enumerate(synthetic_frames(w, h)):
        V = hm.view_constants(cam, w, h)
        model = hm.advance(model, vprev, V, N, a, m, aov, PARAMS, w, h)
        vprev = V
        got_map = hist.advance(cam, N, a, m, aov, want_map=True)
        assert np.array_equal(got_map, model["map"]), (size, k, np.flatnonzero(got_map != model["map"])[:8])
        check_state(hist, model, aov, (size, k))
        seen |= set(np.unique(model["map"][model["map"] < 0]).tolist())
        taps |= set(np.unique(model["tap"]).tolist())
        info = hist.info
        assert (info.frames, info.last_samples, info.min_count, info.max_count) == (k + 1, N, int(model["count"].min()), int(model["count"].max()))
    if w * h > 256:      # the large case meets every way a pixel ends, a source in the footprint's other taps and the cap
        assert {-1, -2, -3, -5, -6} <= seen and {0, 1, 2} <= taps, (seen, taps)
        assert model["count"].max() == PARAMS.max_samples + N and (model["map"] >= 0).any()
    hist.close()


@pytest.mark.parametrize("corner", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_a_primary_tap_in_a_corner_with_the_footprint_outside_the_image(pta, corner):
    """tests/test_history_model.py's corner case: the corner pixel of the previous view belongs to another surface (the wall
    has a hole there), the taps move towards the corner, so the kernel is asked for neighbours that do not exist."""
    w, h = 3, 2
    cx, cy = corner[0] * (w - 1), corner[1] * (h - 1)
    sgn = (1 if corner[0] else -1), (-1 if corner[1] else 1)
    hole = [((0.0, 0.0, -4.0), (0.0, 0.0, 1.0), lambda P: ~((P[:, 0] * sgn[0] > 1.0) & (P[:, 1] * sgn[1] > 0.5)))]
    wall = [((0.0, 0.0, -4.0), (0.0, 0.0, 1.0), None)]
    eps = 0.02 * sgn[0], 0.02 * sgn[1]
    moved = hm.look_at((0.0, 0.0, 0.0), (eps[0], eps[1], -1.0), fov=0.9)
    frames = synthetic_frames(w, h, (FRONT,), hole) + synthetic_frames(w, h, (moved,), wall)
    assert frames[0][3][cx + cy * w, 7] == 0 and (frames[0][3][:, 7] > 0).sum() == w * h - 1
    hist = pta.History(w, h, hparams(pta, PARAMS))
    model, vprev = None, None
    for k, (cam, a, m, aov) in enumerate(frames):
        V = hm.view_constants(cam, w, h)
        model = hm.advance(model, vprev, V, N, a, m, aov, PARAMS, w, h)
        vprev = V
        got_map = hist.advance(cam, N, a, m, aov, want_map=True)
        assert np.array_equal(got_map, model["map"]), (corner, k)
        check_state(hist, model, aov, (corner, k))
    assert model["map"][cx + cy * w] == -4 and model["count"][cx + cy * w] == N
    assert (np.delete(model["map"], cx + cy * w) == np.delete(np.arange(w * h), cx + cy * w)).all()
    hist.close()


def test_a_sparse_previous_view_is_reached_through_every_tap_of_the_footprint(pta):
    """The previous view has a surface only where x and y are odd; the camera then turns by a twentieth of a pixel: an (even,
    even) pixel finds its source in the diagonal tap, the others in the second or third, the (odd, odd) ones in the first."""
    w, h = 9, 6
    wall = [((0.0, 0.0, -4.0), (0.0, 0.0, 1.0), None)]
    (cam0, a0, m0, aov0), = synthetic_frames(w, h, (FRONT,), wall)
    ys, xs = np.divmod(np.arange(w * h), w)
    aov0[~((xs % 2 == 1) & (ys % 2 == 1))] = 0
    aov0[~((xs % 2 == 1) & (ys % 2 == 1)), 14] = np.int32(-1).view(f32)
    moved = hm.look_at((0.0, 0.0, 0.0), (0.004, -0.004, -1.0), fov=0.9)
    (cam1, a1, m1, aov1), = synthetic_frames(w, h, (moved,), wall)
    hist = pta.History(w, h, hparams(pta, PARAMS))
    model, vprev = None, None
    for k, (cam, a, m, aov) in enumerate(((cam0, a0, m0, aov0), (cam1, a1, m1, aov1))):
        V = hm.view_constants(cam, w, h)
        model = hm.advance(model, vprev, V, N, a, m, aov, PARAMS, w, h)
        vprev = V
        got_map = hist.advance(cam, N, a, m, aov, want_map=True)
        assert np.array_equal(got_map, model["map"]), k
        check_state(hist, model, aov, k)
    tap = model["tap"].reshape(h, w)
    assert {0, 1, 2, 3} == set(np.unique(tap[tap >= 0]).tolist()) and (tap >= 0).sum() > w * h // 2
    assert (tap[1::2, 1::2] == 0).all() and (tap[0::2, 0::2][tap[0::2, 0::2] >= 0] == 3).all()
    hist.close()


def test_the_device_form_on_torch_tensors(pta):
    import torch
    w, h = 37, 23
    n = w * h
    hist = pta.History(w, h, hparams(pta, PARAMS))
    stream = torch.cuda.current_stream().cuda_stream
    model, vprev = None, None
    for k, (cam, a, m, aov) in enumerate(synthetic_frames(w, h)):
        V = hm.view_constants(cam, w, h)
        model = hm.advance(model, vprev, V, N, a, m, aov, PARAMS, w, h)
        vprev = V
        d_a, d_m, d_aov = (torch.from_numpy(x.copy()).cuda() for x in (a, m, aov))
        d_map = torch.full((n + 16,), -77, dtype=torch.int32, device="cuda")
        hist.advance_device(cam, N, d_a.data_ptr(), d_m.data_ptr(), d_aov.data_ptr(), d_map.data_ptr() if k != 1 else None, stream=stream)
        torch.cuda.synchronize()
        got = d_map.cpu().numpy()
        assert (got[n:] == -77).all()
        assert np.array_equal(got[:n], model["map"]) if k != 1 else (got == -77).all()
        check_state(hist, model, aov, k)
    # resolve and the filter through their device forms
    acc, mom, cnt, surf, guides = hist.read()
    d_rgb = torch.zeros(n * 3, dtype=torch.uint8, device="cuda")
    d_col = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
    hist.resolve_device("ACES", d_rgb.data_ptr(), d_col.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    rgb, col = hist.resolve("ACES")
    assert same_bits(d_col.cpu().numpy().reshape(-1, 3), col) and np.array_equal(d_rgb.cpu().numpy().reshape(-1, 3), rgb)
    params = pta.DenoiseParams.default_var(iterations=2)
    hist.denoise_device(params, 1, d_rgb.data_ptr(), d_col.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    col, rgb = hist.denoise(params, True)
    assert same_bits(d_col.cpu().numpy().reshape(-1, 3), col) and np.array_equal(d_rgb.cpu().numpy().reshape(-1, 3), rgb)
    assert len(hist.kernel_times(3)) == 3
    check_state(hist, model, aov, "after the timings")
    hist.close()


def test_get_view_equals_the_view_constants(pta):
    import scene_builder as sb
    w, h = 24, 16
    hist = pta.History(w, h)
    with pytest.raises(pta.PtError):
        hist.view(1)
    cams = [sb.make_camera(pta), sb.make_camera(pta, eye=(1.7, 0.3, -2.2), target=(0.0, 0.5, 0.1), fov=0.61), sb.make_camera(pta, eye=hm.orbit_eye(5))]
    a, m = hm.noise_planes(w * h, N, 3)
    aov = np.zeros((w * h, 16), f32)
    for k, cam in enumerate(cams):
        hist.advance(cam, N, a, m, aov)
        for which, c in ((1, cam), (0, cams[max(k - 1, 0)])):
            V, got = hm.view_constants(c, w, h), hist.view(which)
            M = np.array(list(got.M), f32).reshape(3, 3)
            assert same_bits(M, V.M) and same_bits(np.array(list(got.c3), f32), V.c3)
            assert same_bits(np.array([got.tx, got.ty], f32), np.array([V.tx, V.ty], f32))
            t, _ = hm.camera_fields(c)
            A = np.array([[t[4 * j + r] for j in range(3)] for r in range(3)], float)
            assert np.abs(M.astype(float) @ A - np.eye(3)).max() <= 1e-6
    hist.close()


# ------------------------------------------------------------------------------------------------ resolve and the filter
@pytest.fixture(scope="module")
def filled(pta):
    """A history after the three synthetic frames at 37 x 23 (counts 4, 8 and 10), with its planes."""
    w, h = 37, 23
    hist = pta.History(w, h, hparams(pta, PARAMS))
    for cam, a, m, aov in synthetic_frames(w, h):
        hist.advance(cam, N, a, m, aov)
    yield hist, (w, h), hist.read(), aov
    hist.close()


def test_resolve_equals_the_non_uniform_film_resolve(pta, oracle, filled):
    hist, (w, h), (acc, mom, cnt, surf, guides), aov = filled
    assert len(np.unique(cnt)) >= 3
    want = (acc / cnt[:, None].astype(f32)).astype(f32)
    for tm in ("REINHARD", "FILMIC", "ACES"):
        rgb, col = hist.resolve(tm)
        assert same_bits(col, want)
        assert np.array_equal(rgb, oracle.post_process(pta.Profile.make(w, h, 1, 1, tm), want)), tm


@pytest.mark.parametrize("variance", [0, 1])
def test_denoise_equals_the_film_filter_model(pta, oracle, filled, variance):
    hist, (w, h), (acc, mom, cnt, surf, guides), aov = filled
    guides = am.guides_of(aov, N)
    valid = guides[:, 3] >= 0
    assert valid.any() and (~valid).any()
    for k, (it, fl) in enumerate(((0, 0), (1, pta.PT_DENOISE_NO_DEMODULATE), (3, 0))):
        make = pta.DenoiseParams.default_var if variance else pta.DenoiseParams.default
        params = make(iterations=it, flags=fl, tonemap=k % 3)
        want, _ = fdm.film_denoise_with(params, w, h, cnt, acc, mom, guides, bool(variance))
        col, rgb = hist.denoise(params, bool(variance))
        assert same_bits(col, want), (variance, it, fl, int((bits(col) != bits(want)).any(axis=1).sum()))
        assert np.array_equal(rgb, oracle.post_process(pta.Profile.make(w, h, 1, 1, int(params.tonemap)), want))
        if it:
            assert not same_bits(col[valid], hist.resolve()[1][valid])


# ------------------------------------------------------------------------------------------------ add_frame
def e2e_frames(pta, g, rotate):
    """[(camera, accum, moments, aov)] of the three orbit frames from pt_render_window / pt_render_moments and pt_render_aov."""
    out = []
    w, h = hm.E2E_SIZE
    for k in range(3):
        _, camera, prof = hm.e2e_scene(pta, k)
        g.set_camera(camera)
        if rotate == 1:
            _, acc, mom = g.render_moments(prof)
        else:
            wide = pta.Profile.make(w, h, rotate * N, prof.bounces, prof.tonemap)
            j = k % rotate
            zero_a, zero_m = np.zeros((w * h, 3), f32), np.zeros((w * h, 2), f32)
            _, acc, mom = g.render_window(wide, j * N, j * N + N, accum=zero_a, moments=zero_m)
        out.append((camera, acc, mom, g.render_aov(prof)))
    return out


@pytest.mark.parametrize("rotate", [2, 1])
def test_add_frame_equals_the_model_on_the_orbit(pta, rotate):
    w, h = hm.E2E_SIZE
    assert hm.E2E_SAMPLES == N
    scene, _, prof = hm.e2e_scene(pta, 0)
    g = pta.GpuScene(scene)
    params = hm.DEFAULTS._replace(rotate=rotate)
    frames = e2e_frames(pta, g, rotate)
    hist = pta.History(w, h, hparams(pta, params))
    model, vprev = None, None
    for k, (camera, acc, mom, aov) in enumerate(frames):
        V = hm.view_constants(camera, w, h)
        model = hm.advance(model, vprev, V, N, acc, mom, aov, params, w, h)
        vprev = V
        g.set_camera(camera)
        hist.add_frame(g, prof, k)
        check_state(hist, model, aov, (rotate, k))
        if k:
            share = hm.share(model["map"], model["surf"])
            print(f"rotate {rotate} frame {k}: {share:.3f} of the surface pixels find a source")
            assert share >= 0.5, (rotate, k, share)
    assert model["count"].max() == 3 * N
    hist.close()
    g.close()


def counters(g):
    i = g.info()
    return (g.rng_cache_stats(), g.hit_cache_stats(), g.hit1_cache_stats(), (i.frame_planned, i.queue_chunk_items, i.queue_bytes))


def test_add_frame_leaves_the_scenes_steady_state_as_plain_frames_do(pta):
    w, h = hm.E2E_SIZE
    scene, camera, prof = hm.e2e_scene(pta, 0)
    # rotate 1: frame, add_frame, frame == three plain frames
    plain, mixed = pta.GpuScene(scene), pta.GpuScene(scene)
    hist = pta.History(w, h, hparams(pta, hm.DEFAULTS._replace(rotate=1)))
    for k in range(3):
        want = plain.render(prof)
        if k == 1:
            hist.add_frame(mixed, prof, k)
            got_acc = hist.read()[0]
        else:
            got_acc = mixed.render(prof)[1]
        assert same_bits(got_acc, want[1]), k
        assert counters(mixed) == counters(plain), k
    hist.close()
    # rotate > 1: a window frame moves no counter and the frame behind it follows its predecessor
    hist = pta.History(w, h, hparams(pta, hm.DEFAULTS._replace(rotate=2)))
    for _ in range(4):
        before = mixed.render(prof)
    c0 = counters(mixed)
    hist.add_frame(mixed, prof, 1)
    assert counters(mixed) == c0
    after = mixed.render(prof)
    assert same_bits(before[1], after[1]) and np.array_equal(before[0], after[0])
    hist.close()
    plain.close()
    mixed.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_what_a_history_refuses_leaves_it_unchanged(pta):
    w, h = 8, 4
    n = w * h
    for bad in (dict(max_samples=0), dict(max_samples=MAX), dict(rotate=0), dict(normal_cos=float("nan")), dict(plane_tol=-1.0)):
        with pytest.raises(pta.PtError) as e:
            pta.History(w, h, pta.HistoryParams.default(**bad))
        assert e.value.code == pta.PT_ERR_INVALID, bad
    with pytest.raises(pta.PtError):
        pta.History(0, 4)
    hist = pta.History(w, h, pta.HistoryParams.default(max_samples=MAX - 8))
    (cam, a, m, aov), = synthetic_frames(w, h, (FRONT,))
    # an empty history: nothing to resolve or filter
    for call in (lambda: hist.resolve(), lambda: hist.denoise(pta.DenoiseParams.default(), False), lambda: hist.kernel_times(1)):
        with pytest.raises(pta.PtError) as e:
            call()
        assert e.value.code == pta.PT_ERR_INVALID and "no samples" in str(e.value)
    hist.advance(cam, 1, a, m, aov)                 # one sample: a variance needs two
    before = hist.read()
    singular = dict(FRONT, transform=[[1, 0, 0, 0], [2, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    scene, _, prof = hm.e2e_scene(pta, 0)
    g = pta.GpuScene(scene)
    small = pta.Profile.make(w, h, N, 1, "FILMIC")
    refused = [
        (lambda: hist.advance(cam, 0, a, m, aov), pta.PT_ERR_INVALID),
        (lambda: hist.advance(cam, 9, a, m, aov), pta.PT_ERR_INVALID),                      # max_samples + N > 2^24
        (lambda: hist.advance(singular, N, a, m, aov), pta.PT_ERR_INVALID),
        (lambda: hist.advance(None, N, a, m, aov), pta.PT_ERR_INVALID),
        (lambda: hist.advance_device(cam, N, 0, 0, 0), pta.PT_ERR_INVALID),
        (lambda: hist.denoise(pta.DenoiseParams.default_var(), True), pta.PT_ERR_INVALID),
        (lambda: hist.denoise(pta.DenoiseParams.default(iterations=9), False), pta.PT_ERR_INVALID),
        (lambda: hist.denoise(pta.DenoiseParams.default(), False, lum_floor=0.0), pta.PT_ERR_INVALID),
        (lambda: hist.resolve(7), pta.PT_ERR_INVALID),
        (lambda: hist.add_frame(g, small, 0, pta.Opts.make(flags=PT_FLAG_MEGAKERNEL)), pta.PT_ERR_UNSUPPORTED),
        (lambda: hist.add_frame(g, small, 0, pta.Opts.make(shard_rank=0, shard_count=2, tile_w=16, tile_h=16)), pta.PT_ERR_UNSUPPORTED),
        (lambda: hist.add_frame(g, prof, 0), pta.PT_ERR_INVALID),                           # another image size
        (lambda: hist.add_frame(g, pta.Profile.make(w, h, 0, 1, "FILMIC"), 0), pta.PT_ERR_INVALID),
    ]
    for k, (call, code) in enumerate(refused):
        with pytest.raises(pta.PtError) as e:
            call()
        assert e.value.code == code, (k, str(e.value))
        after = hist.read()
        assert all(same_bits(x, y) for x, y in zip(before, after)), k
        assert (hist.info.frames, hist.info.last_samples) == (1, 1), k
    hist.reset()
    assert hist.info.frames == 0 and (hist.read()[2] == 0).all()
    hist.advance(cam, N, a, m, aov)
    assert (hist.read()[2] == N).all()              # the history before the reset is gone
    g.close()
    hist.close()
