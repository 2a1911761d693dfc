"""The clouds planner (plan_clouds, csrc/clouds_plan.cpp) without a GPU: soc_debug_plan_clouds writes what
soc_cloud_rendering would issue for a call (a header with the call's scalars, then the counter-block clears and every
kernel with its instantiation, grid and block, in issue order, then the renderer's CloudState as the call leaves it).

Every call of every case is compared, byte for byte, with tests/golden/cloud_plans.json. Those texts were recorded from
the commit before the planner existed, not from the planner: a scratch copy of that commit's clouds.hip, compiled with
that file's flags, linked with that commit's other objects and run on the CPU, in which `launch`, `hipMemsetAsync`,
`check_launch` and `resident_blocks` were replaced, ahead of the host section, by recorders. The launch recorder
appends the kernel line (it names the instantiation by looking the kernel's host pointer up in a table of the 33, and
reads clouds_od_lut's table pointer and lut_blocks from the arguments), the memset recorder names the counter block by
its address in the workspace layout, and resident_blocks returns the injected residency of the instantiation it is
asked about (another than the six aborts). One statement ahead of each of the launcher's two returns after launches
formats the header line from the launcher's own locals (W, H, ws.pb.n, counter, zero_next, vec_store, ws.pb, lut, C2, st), and
the hook around soc::cloud_rendering_launch adds the state line. This module's own cases drove that library through
the same hook signature (record() below), so a case added later needs the same kind of recording to get its golden.

The fixture stores each distinct line once ("lines") and every call as [return code, error message, line indices]."""
import ctypes as C
import json
import os

import pytest

from soc_real_time_renderer_amd import _abi

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "cloud_plans.json")
R8, RGBA8, D32F, RGBA16F = _abi.FMT_R8_UNORM, _abi.FMT_RGBA8_UNORM, _abi.FMT_D32F, _abi.FMT_RGBA16F
# six distinct primes (atmosphere, density, sunvis wide / quads / rows, resolve): every cap is visible in a grid
RESIDENCY = (C.c_int32 * 6)(1531, 1543, 769, 773, 787, 1277)
# fake addresses, never dereferenced; 256-byte aligned like real allocations
DEPTH, NOISE, TARGET, WS, WS2 = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000


def call(size=(64, 36), res=None, fmt=RGBA8, ws=WS, sky_bound=0, env=None, sun=None, cam=None, noise=None, target=None,
         depth_fmt=D32F, target_fmt=RGBA8, null_globals=False):
    """One soc_cloud_rendering call: target extent, globals resolution (default: the same), noise format, workspace,
    knobs; noise / target: overrides of (data, width, height, pitch)."""
    return dict(size=size, res=res or size, fmt=fmt, ws=ws, sky_bound=sky_bound, env=env or {}, sun=sun, cam=cam,
                noise=noise or {}, target=target or {}, depth_fmt=depth_fmt, target_fmt=target_fmt, null_globals=null_globals)


def knob(**env):
    return [call(size=(1920, 1080), env={"SOC_CLOUDS_" + k: str(v) for k, v in env.items()})]


PAIR_NINE = [dict(ATMOS_POS=p, GEOM=g, NOISE_TABLE=n, SUNVIS_WIDE=w, DENSITY_ROWS=0 if w == 0 else 1, OD_LUT=0)
             for p, g, n, w in ((0, 1, 1, 2), (1, 1, 1, 2), (2, 1, 1, 2), (2, 0, 1, 2), (2, 1, 0, 2), (2, 1, 1, 1), (2, 1, 0, 1),
                                (2, 1, 1, 0), (2, 1, 0, 0))]
PAIR_FIVE = [dict(ATMOS_POS=2, GEOM=1, NOISE_TABLE=n, RESOLVE_BATCH=rb, DENSITY_BATCH=db, SUNVIS_PF=pf, CLASSIFY_HOIST=h,
                  DENSITY_MULT=2 if h else 1)
             for n, rb, db, pf, h in ((1, 4, 8, 1, 0), (0, 4, 4, 1, 1), (1, 1, 1, 0, 0), (1, 8, 8, 1, 1), (1, 4, 1, 0, 0))]
SUN2 = (0.3, -0.8, 0.4)   # an edited sun: another dot(pSun, pSun)
GOOD = dict(size=(320, 180))

# name -> (with a CloudState, [calls in order])
CASES = {
    "no_workspace": (False, [call(size=s, fmt=f, ws=None) for f in (R8, RGBA8) for s in ((64, 36), (97, 55))]),
    "stateless_defaults": (False, [call(size=(64, 36)), call(size=(1920, 1080)), call(size=(3840, 2160)),
                                   call(size=(2560, 1440), res=(1920, 1080))]),
    "alignment": (False, [call(size=(97, 55), target=dict(pitch=97 * 4 + 4)), call(size=(97, 55), target=dict(data=TARGET + 4))]),
    "rule_1440p": (False, [call(size=s, sky_bound=b) for s in ((2560, 1440), (2562, 1440)) for b in (0, 1)]),
    "rule_1440p_state": (True, [call(size=s, sky_bound=b) for s in ((2560, 1440), (2562, 1440)) for b in (0, 1)]),
    # the default fold leaves no atmosphere kernel to place: the position shows with SOC_CLOUDS_ATMOS_FOLD=0
    "rule_1440p_no_fold": (False, [call(size=s, sky_bound=b, env={"SOC_CLOUDS_ATMOS_FOLD": "0"})
                                   for s in ((2560, 1440), (2562, 1440)) for b in (0, 1)]),
    "atmos_pos": (False, knob(ATMOS_POS=0) + knob(ATMOS_POS=1) + knob(ATMOS_POS=2)),
    "atmos_pos_no_fold": (False, knob(ATMOS_POS=0, ATMOS_FOLD=0) + knob(ATMOS_POS=1, ATMOS_FOLD=0)
                          + knob(ATMOS_POS=2, ATMOS_FOLD=0)
                          + [call(size=(2562, 1440), env={"SOC_CLOUDS_ATMOS_POS": "0", "SOC_CLOUDS_ATMOS_FOLD": "0"})]),
    "geom_0": (False, knob(GEOM=0)),
    "od_lut_0": (False, knob(OD_LUT=0)),
    "noise_table_0": (False, knob(NOISE_TABLE=0)),
    "static_tables": (True, knob(STATIC_TABLES=0) + knob(STATIC_TABLES=1)),
    "classify_hoist_1": (False, knob(CLASSIFY_HOIST=1)),
    "grid_mult": (False, knob(GRID_MULT=1) + knob(GRID_MULT=3)),
    "sky_table_0": (False, knob(SKY_TABLE=0)),
    "atmos_fold_0": (False, knob(ATMOS_FOLD=0)),
    "resolve_batch": (False, knob(RESOLVE_BATCH=1) + knob(RESOLVE_BATCH=8) + knob(RESOLVE_BATCH=5)),
    "density_batch": (False, knob(DENSITY_ROWS=0, DENSITY_BATCH=1) + knob(DENSITY_ROWS=0, DENSITY_BATCH=4)
                      + knob(DENSITY_ROWS=0, DENSITY_BATCH=8)),
    "sunvis_wide": (False, knob(SUNVIS_WIDE=0) + knob(SUNVIS_WIDE=1) + knob(SUNVIS_WIDE=2) + knob(SUNVIS_WIDE=1, SUNVIS_PF=0)),
    "density_mult_2": (False, knob(DENSITY_MULT=2)),
    "pair_path_nine": (False, [call(size=(320, 180), fmt=f, env={"SOC_CLOUDS_" + k: str(v) for k, v in e.items()})
                               for f in (R8, RGBA8) for e in PAIR_NINE]),
    "pair_path_five": (False, [call(size=(320, 180), fmt=f, env={"SOC_CLOUDS_" + k: str(v) for k, v in e.items()})
                               for f in (R8, RGBA8) for e in PAIR_FIVE]),
    # three equal frames (the build in the first only, the blocks alternate), then each key changed alone
    "state_keys": (True, [call(**GOOD)] * 3 + [call(sun=SUN2, **GOOD),
                                                call(sun=SUN2, noise=dict(data=NOISE + 4096), **GOOD),
                                                call(sun=SUN2, noise=dict(data=NOISE + 4096, pitch=256), fmt=R8, **GOOD),
                                                call(sun=SUN2, noise=dict(data=NOISE + 4096, pitch=512), fmt=R8, **GOOD),
                                                call(sun=SUN2, noise=dict(data=NOISE + 4096, pitch=512), fmt=R8, ws=WS2, **GOOD)]),
    "state_static_tables_0_between": (True, [call(**GOOD), call(env={"SOC_CLOUDS_STATIC_TABLES": "0"}, **GOOD), call(**GOOD)]),
    "state_failed_frame_between": (True, [call(**GOOD), call(noise=dict(height=32), **GOOD), call(**GOOD)]),
    "sky_table_edges": (False, [call(size=(320, 180), sun=(0.0, -1.0, 0.0), cam=(0.0, 2.0, 0.0)),
                                call(size=(320, 180), sun=(0.0, 0.0, -1.0), cam=(0.0, -6372e3, 7000e3)),
                                call(size=(320, 180), cam=(-14.0, -1500.0, 0.3))]),
    "refusals": (True, [call(null_globals=True), call(depth_fmt=RGBA16F), call(target_fmt=R8), call(fmt=RGBA16F),
                        call(noise=dict(width=32)), call(size=(65536, 1)), call(res=(0, 36))]),
}
BPP = {R8: 1, RGBA8: 4, D32F: 4, RGBA16F: 8}


def run_case(soc, name, setenv, delenv):
    """[(return code, error message, text)] of the case's calls, in order, on one CloudState (or none)."""
    lib = soc.lib()
    with_state, calls = CASES[name]
    state = C.create_string_buffer(lib.soc_debug_cloud_state_bytes()) if with_state else None
    out = []
    for c in calls:
        for k, v in c["env"].items():
            setenv(k, v)
        lib.soc_tuning_reload()
        (w, h), (gw, gh) = c["size"], c["res"]
        g = soc.globals_defaults(max(gw, 1), max(gh, 1))
        g.resolution[0], g.resolution[1] = gw, gh
        g.elapsed_time = 10.0
        if c["sun"]:
            g.sun_info.direction[:] = c["sun"]
        if c["cam"]:
            g.camera_position[:] = c["cam"]

        def image(data, w, h, fmt, over):
            return soc.SocImg(over.get("data", data), over.get("width", w), over.get("height", h),
                              over.get("pitch", w * BPP[fmt]), fmt)
        buf = C.create_string_buffer(4096)
        n = lib.soc_debug_plan_clouds(None if c["null_globals"] else C.byref(g), image(DEPTH, w, h, c["depth_fmt"], {}),
                                      image(NOISE, 64, 64, c["fmt"], c["noise"]), image(TARGET, w, h, c["target_fmt"], c["target"]),
                                      c["ws"], c["sky_bound"], RESIDENCY, state, buf, len(buf))
        assert n < len(buf)
        text = buf.value.decode()
        assert n < 0 or n == len(text)
        out.append((min(n, 0), lib.soc_last_error_string().decode() if n < 0 else "", text))
        for k in c["env"]:
            delenv(k)
    lib.soc_tuning_reload()
    return out


def record(soc, path):
    """Writes the fixture from `soc`'s library: run on the recording library described above, never on the planner."""
    lines, cases = [], {}
    for name in CASES:
        cases[name] = []
        for rc, msg, text in run_case(soc, name, os.environ.__setitem__, os.environ.__delitem__):
            idx = []
            for line in text.splitlines(keepends=True):
                if line not in lines:
                    lines.append(line)
                idx.append(lines.index(line))
            cases[name].append([rc, msg, idx])
    with open(path, "w") as f:
        f.write('{"lines": [\n' + ",\n".join(json.dumps(s) for s in lines) + '],\n"cases": {\n'
                + ",\n".join(json.dumps(k) + ": " + json.dumps(v) for k, v in cases.items()) + "}}\n")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fixture_covers_the_cases(golden):
    assert sorted(golden["cases"]) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_plans_are_the_recorded_ones(soc, golden, monkeypatch, name):
    got = run_case(soc, name, monkeypatch.setenv, monkeypatch.delenv)
    want = [(rc, msg, "".join(golden["lines"][i] for i in idx)) for rc, msg, idx in golden["cases"][name]]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, k)


def test_recorded_plans_show_what_the_cases_are_about(golden):
    """The fixture itself: the properties the cases were chosen for are in the recorded texts."""
    def steps(name, k):
        rc, _, idx = golden["cases"][name][k]
        return rc, [golden["lines"][i].rstrip("\n").split("\t") for i in idx]
    kinds = lambda st: [s[1] if s[0] == "kernel" else s[0] for s in st]
    # three equal frames: primed and built in the first only, the blocks alternate, the other block is zeroed
    f = [steps("state_keys", k)[1] for k in range(8)]
    assert kinds(f[0])[:4] == ["clouds", "memset", "memset", "clouds_od_lut"]
    assert all("memset" not in kinds(x) and "clouds_od_lut" not in kinds(x) for x in f[1:3])
    assert [(x[0][4], x[0][5]) for x in f[:3]] == [("counter=0", "zero=1"), ("counter=1", "zero=0"), ("counter=0", "zero=1")]
    # a changed sun rebuilds the od table alone, a changed noise key the noise tables alone, another workspace re-primes
    assert [s[2].split(" ", 1)[1].rsplit(" ", 1)[0] for s in f[3] if s[1] == "clouds_od_lut"] == ["od=1 noise=0"]
    for x in f[4:7]:
        assert [s[2].split(" ", 1)[1].rsplit(" ", 1)[0] for s in x if s[1] == "clouds_od_lut"] == ["od=0 noise=1"]
    assert kinds(f[7])[:4] == ["clouds", "memset", "memset", "clouds_od_lut"]
    # a failed frame and a per-call frame each leave a state that the next frame re-primes and rebuilds from
    for name in ("state_failed_frame_between", "state_static_tables_0_between"):
        assert kinds(steps(name, 2)[1])[:4] == ["clouds", "memset", "memset", "clouds_od_lut"]
    assert steps("state_failed_frame_between", 1)[0] == -2
    # the 1440p rule: above it the atmosphere follows the sun visibility, and a sky-bound frame builds per call
    below, above = kinds(steps("rule_1440p_state", 1)[1]), kinds(steps("rule_1440p_state", 3)[1])
    assert "memset" in kinds(steps("rule_1440p_state", 0)[1]) and "clouds_od_lut" not in below
    assert "clouds_od_lut" in above and steps("rule_1440p_state", 3)[1][0][5] == "zero=-1"
    march = ["clouds_density", "clouds_sunvis", "clouds_resolve"]
    order = lambda name, k: [x for x in kinds(steps(name, k)[1]) if x in march + ["clouds_atmosphere"]]
    for k in (0, 1):   # 2560x1440, either lane priority: the atmosphere first
        assert order("rule_1440p_no_fold", k) == ["clouds_atmosphere"] + march
    for k in (2, 3):   # 2562x1440: after the sun visibility
        assert order("rule_1440p_no_fold", k) == march[:2] + ["clouds_atmosphere"] + march[2:]
    assert [order("atmos_pos_no_fold", k).index("clouds_atmosphere") for k in range(4)] == [0, 1, 2, 0]
    assert all("clouds_atmosphere" not in kinds(steps("atmos_pos", k)[1]) for k in range(3))   # folded: nothing to place
    # the workspace is laid out for the target's extent, W and H are the smaller of the target's and the globals'
    assert steps("stateless_defaults", 3)[1][0][1:4] == ["1920", "1080", "list=%d" % (2560 * 1440)]
    # no sky table below the surface, hence the atmosphere kernel; both zenith fallbacks keep the table
    assert "clouds_atmosphere" in kinds(steps("sky_table_edges", 2)[1])
    assert all("clouds_sky_table" in kinds(steps("sky_table_edges", k)[1]) for k in (0, 1))
    assert [steps("refusals", k)[0] for k in range(7)] == [-1, -1, -1, -4, -2, -2, 0]
