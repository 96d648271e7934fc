"""The cached opaque bounce-0 kernel at four waves per SIMD (csrc/pt_wavefront.h: k_wf_shade<..., GRID 3 + 8>, WF_SHADE_PARK,
wf_opaque_arg): the state that is cold across the inline shadow casts waits in LDS, and the kernel's arguments are read through
a pointer the compiler cannot see through, so that nothing derived from them is hoisted into registers for the whole loop.

What could go wrong: a register count or a scratch size that silently takes the fourth wave away again (the code object is
read), an LDS size that keeps the fourth workgroup off the CU (the runtime is asked), a parked value that comes back wrong or
an argument read at the wrong offset of the kernarg segment - then no cached frame is the uncached frame any more.  Every
cached frame here is compared bit for bit, f32 accumulator and rgb8, with the CPU oracle and with a PT_RNG_CACHE=0 render,
and every case reads the cache's own numbers: without them it would not prove that the cached variant ran."""
import hashlib
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
LLVM = Path("/opt/rocm/lib/llvm/bin")
gpu = pytest.mark.gpu


# ---------------------------------------------------------------- the code object (as tests/test_kernel_resources.py reads it)
def kernel_table(tmp_path):
    import re
    import shutil
    lib = ROOT / "path-tracer_amd" / "libptgpu.so"
    tools = [LLVM / "clang-offload-bundler", LLVM / "llvm-readelf", shutil.which("objcopy")]
    if not lib.exists() or not all(t and Path(t).exists() for t in tools):
        pytest.skip("libptgpu.so or the LLVM binutils are not here")
    fat, elf = tmp_path / "fat.bin", tmp_path / "gfx950.elf"
    subprocess.run([tools[2], "-O", "binary", "--only-section=.hip_fatbin", str(lib), str(fat)], check=True)
    subprocess.run([str(tools[0]), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    f"--input={fat}", f"--output={elf}"], check=True)
    notes = subprocess.run([str(tools[1]), "--notes", str(elf)], check=True, capture_output=True, text=True).stdout
    table = {}
    for block in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        table[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                       for k in ("private_segment_fixed_size", "vgpr_count", "sgpr_count", "group_segment_fixed_size")}
    return table


def find(table, fragment):
    hits = [v for k, v in table.items() if fragment in k]
    assert len(hits) == 1, (fragment, [k for k in table if fragment in k])
    return hits[0]


def test_cached_variants_fit_four_waves_without_scratch(tmp_path):
    """128 registers are four waves per SIMD; 16 B of scratch is the allowance (the three-wave kernel had 8, by launch
    bounds alone four waves cost 180 and 3.4 ms of the frame); 40 KiB of LDS are a quarter of a CU's 160 KiB.  The variant
    with the orthographic branch (directional lights) is held to the same limits; the uncached variant keeps its budget."""
    t = kernel_table(tmp_path)
    for variant in ("k_wf_shadeILb0ELb0ELb1ELi11EE", "k_wf_shadeILb0ELb0ELb1ELi15EE"):
        k = find(t, variant)
        print(variant, k)
        assert k["vgpr_count"] <= 128, (variant, k)
        assert k["private_segment_fixed_size"] <= 16, (variant, k)
        assert k["group_segment_fixed_size"] <= 40960, (variant, k)
    b0 = find(t, "k_wf_shadeILb0ELb0ELb1ELi3EE")
    print("uncached", b0)
    assert b0["vgpr_count"] <= 170 and b0["private_segment_fixed_size"] <= 32, b0
    # the parking array belongs to the two variants above alone: every other bounce-0 variant keeps the compaction's 296 B of
    # LDS (two wave counts, two bases, the octant tables), the later bounces' variants add the hit aggregation to it
    import re
    seen = 0
    for name, k in t.items():
        m = re.search(r"k_wf_shadeILb([01])ELb([01])ELb([01])ELi(\d+)EE", name)
        if not m or (m.group(1), m.group(2), m.group(3), m.group(4)) in (("0", "0", "1", "11"), ("0", "0", "1", "15")):
            continue
        seen += 1
        limit = 296 if m.group(3) == "1" else 6456   # PRIMARY: bounce 0
        assert k["group_segment_fixed_size"] <= limit, (name, k)
    assert seen >= 10, seen


@gpu
def test_the_runtime_places_four_workgroups_per_cu(pta):
    cached, uncached = pta.kernel_occupancy(1), pta.kernel_occupancy(0)
    print("workgroups per CU: cached", cached, "uncached", uncached)
    assert cached >= 4, cached
    assert uncached >= 3, uncached


# ---------------------------------------------------------------- bit identity of the cached frames
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "rgb8", int((got[0] != want[0]).any(axis=1).sum()))
    same = bits(got[1]) == bits(want[1])
    assert same.all(), (what, "accum", int((~same).any(axis=1).sum()), "first", np.argwhere(~same)[0].tolist())


def stats(g):
    return dict(zip(("bytes", "items", "cached", "fills"), g.rng_cache_stats()))


_oracle_frames = {}


def oracle_frame(oracle, key, scene, prof):
    """The brute-force oracle's frame, made once per (scene, profile) and shared."""
    if key not in _oracle_frames:
        rgb, acc, _ = oracle.OracleScene(scene.desc, oracle.PTO_BRUTE_FORCE).render(prof)
        rgb.setflags(write=False)
        acc.setflags(write=False)
        _oracle_frames[key] = (rgb, acc)
    return _oracle_frames[key]


def three_frames(pta, monkeypatch, scene, prof, want, what, opts=None, pick=None):
    """A PT_RNG_CACHE=0 render and three consecutive frames of one scene: the second fills the cache, the second and the
    third read it - all of them `want` (pick: the rank's pixels of the whole frame)."""
    if pick is not None:
        want = (want[0][pick], want[1][pick])
    monkeypatch.setenv("PT_RNG_CACHE", "0")
    g = pta.GpuScene(scene)
    assert_same(g.render(prof, opts), want, (what, "PT_RNG_CACHE=0"))
    assert stats(g)["cached"] == 0
    g.close()
    monkeypatch.delenv("PT_RNG_CACHE")
    g = pta.GpuScene(scene)
    for frame in range(3):
        assert_same(g.render(prof, opts), want, (what, "frame", frame))
        st = stats(g)
        if frame == 0:
            assert st["cached"] == 0 and st["fills"] == 0, (what, st)
        else:   # the cached variant ran for every item of the frame
            assert st["items"] > 0 and st["cached"] == st["items"] and st["fills"] == 1, (what, frame, st)
    g.close()


GOLDEN = {"spheres": 4, "head": 4, "white_furnace_direct": 0}   # scene -> bounces (the goldens' own)


@gpu
@pytest.mark.parametrize("name", list(GOLDEN))
def test_golden_scenes(pta, oracle, scene_cache, monkeypatch, name):
    """spheres: the sphere branch of both casts; head: textures and a directional light (the GRID 3 + 4 + 8 variant);
    white_furnace_direct: bounces 0, the path ends in the kernel."""
    scene = scene_cache(name)
    prof = pta.Profile.make(40, 24, 3, GOLDEN[name])
    three_frames(pta, monkeypatch, scene, prof, oracle_frame(oracle, (name, 40, 24, 3), scene, prof), name)


_stand_ins = {}


def stand_in(pta, flags):
    if flags not in _stand_ins:
        _stand_ins[flags] = pta.HostScene.generate_ps5(2000, seed=0, flags=flags)
    return _stand_ins[flags]


SIZES = [(40, 24, 3), (64, 64, 4)]


@gpu
@pytest.mark.parametrize("bounces", [0, 5])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("flags", [8, 9])
def test_generated_scene(pta, oracle, monkeypatch, flags, size, bounces):
    """2 000 triangles in the reference framing, opaque (8) and translucent (9: the ALPHA variant, which keeps three waves):
    the whole frame, and rank 1 of 3 with 16 x 16 tiles."""
    w, h, spp = size
    scene = stand_in(pta, flags)
    prof = pta.Profile.make(w, h, spp, bounces)
    want = oracle_frame(oracle, (flags, size, bounces), scene, prof)
    three_frames(pta, monkeypatch, scene, prof, want, (flags, size, bounces))
    shard = pta.Opts.make(shard_rank=1, shard_count=3, tile_w=16, tile_h=16)
    three_frames(pta, monkeypatch, scene, prof, want, (flags, size, bounces, "shard"), shard, pta.local_pixel_map(prof, shard))


CHILD = r"""
import hashlib, sys
sys.path.insert(0, %(root)r)
import __graft_entry__ as e
pta = e.load_package()
for flags in (8, 9):
    scene = pta.HostScene.generate_ps5(2000, seed=0, flags=flags)
    for (w, h, spp) in %(sizes)r:
        for bounces in (0, 5):
            g = pta.GpuScene(scene, device=0)
            prof = pta.Profile.make(w, h, spp, bounces)
            for frame in range(3):
                rgb, acc = g.render(prof)
                st = g.rng_cache_stats()
                assert frame == 0 or (st[1] > 0 and st[2] == st[1] and st[3] == 1), st
                print("SHA", flags, w, h, spp, bounces, frame, hashlib.sha1(rgb.tobytes() + acc.tobytes()).hexdigest())
            g.close()
"""


@gpu
def test_generated_scene_without_the_camera_cull(pta, oracle):
    """PT_CAM_CULL=0 is read once per process: one child renders every case of the generated scene with the cull off (every
    sample of an empty 8 x 8 block then runs through the kernel); its frames are the oracle's."""
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PT_CAM_", "PT_RNG_"))}
    env["PT_CAM_CULL"] = "0"
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": str(ROOT), "sizes": SIZES}], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln.split()[1:] for ln in out.stdout.splitlines() if ln.startswith("SHA ")]
    assert len(lines) == 2 * len(SIZES) * 2 * 3, out.stdout[-1000:]
    for flags, w, h, spp, bounces, frame, sha in lines:
        size = (int(w), int(h), int(spp))
        scene = stand_in(pta, int(flags))
        want = oracle_frame(oracle, (int(flags), size, int(bounces)), scene, pta.Profile.make(*size, int(bounces)))
        assert sha == hashlib.sha1(want[0].tobytes() + want[1].tobytes()).hexdigest(), (flags, size, bounces, frame)


@gpu
def test_two_frames_in_flight_on_two_streams(pta, oracle):
    """Six frames enqueued without a host wait, alternating between two streams (each waits on the device for the frame
    before it): the second fills the cache, the later ones read it through the four-wave kernel."""
    import torch
    w, h, spp = SIZES[1]
    scene = stand_in(pta, 8)
    prof = pta.Profile.make(w, h, spp, 5)
    want = oracle_frame(oracle, (8, SIZES[1], 5), scene, prof)
    n = w * h
    outs = [(torch.empty(n * 3, dtype=torch.uint8, device="cuda"), torch.empty(n * 3, dtype=torch.float32, device="cuda"))
            for _ in range(6)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    g = pta.GpuScene(scene)
    for k, (rgb, acc) in enumerate(outs):
        st = streams[k & 1]
        st.wait_stream(streams[(k & 1) ^ 1])
        g.render_device(prof, pta.Opts.make(), rgb.data_ptr(), acc.data_ptr(), st.cuda_stream)
    for st in streams:
        st.synchronize()
    for k, (rgb, acc) in enumerate(outs):
        assert_same((rgb.cpu().numpy().reshape(-1, 3), acc.cpu().numpy().reshape(-1, 3)), want, k)
    st = stats(g)
    assert st["items"] > 0 and st["cached"] == st["items"] and st["fills"] == 1, st
    g.close()
