"""The Composition planner (plan_composition / plan_sky_compose, csrc/composition_plan.cpp) without a GPU:
soc_debug_plan_composition writes what a Composition call would issue (a header with the parameter block's scalars and
the bit patterns of its host arithmetic, then every kernel with its form, grid and block, the bloom mips it is given,
whether it gets the light bounds and the counter, then a following histogram pass), or returns the call's error.

Every call of every case is compared, byte for byte, with tests/golden/composition_plans.json. Those texts were
recorded from the commit before the planner existed, not from the planner: a scratch copy of that commit's
composition.hip, compiled with that file's flags and linked with that commit's other objects, in which
`launch`, `check_launch` and `soc_generate_luminance_histogram` were replaced, ahead of the host section, by recorders.
The launch recorder names the instantiation by looking the kernel's host pointer up in a table of the 37, and formats
the header from the parameter block the launcher passes (its local `p`, `pb` or `pc`, as the kernel would receive it;
the histogram's fields only where p.bins is set: the launcher leaves them unset otherwise) and the kernel line from the
grid, the block and the other arguments. A hook of soc_debug_plan_composition's signature called that commit's
composition_launch (calls without the histogram), composition_luminance_histogram (with it) or sky_compose_launch with
the same arguments. This module's own cases drove that library (record() below), so a case added later needs the same
kind of recording to get its golden.

The fixture stores each distinct line once ("lines") and every call as [return code, error message, line indices]."""
import ctypes as C
import json
import math
import os

import pytest

from soc_real_time_renderer_amd import _abi

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "composition_plans.json")
R8, RGBA8, D32F, RGBA16F = _abi.FMT_R8_UNORM, _abi.FMT_RGBA8_UNORM, _abi.FMT_D32F, _abi.FMT_RGBA16F
BPP = {R8: 1, RGBA8: 4, D32F: 4, RGBA16F: 8}
IMAGES = ("target", "albedo", "emissive", "normal", "depth", "ssao", "shadow", "clouds")
FORMATS = dict(target=RGBA16F, albedo=RGBA16F, emissive=RGBA16F, normal=RGBA16F, depth=D32F, ssao=R8, shadow=D32F, clouds=RGBA8)
# fake addresses, never dereferenced; 256-byte aligned like real allocations
BASE = {n: 0x10000000 * (i + 1) for i, n in enumerate(IMAGES)}
MIP1, MIP3, DG, AE, SCRATCH, BOUNDS, COUNTER = 0xa0000000, 0xb0000000, 0xc0000000, 0xc1000000, 0xc2000000, 0xc3000000, 0xc4000000
HIST, FOLD, SKY_EXTERNAL, BOUNDED, CASCADED, SKY_COMPOSE = 1, 2, 4, 8, 16, 32
SHADOW = 256   # the sun's map; a cascaded call's atlas is SHADOW x count * SHADOW


def call(what=0, size=(64, 36), res=None, lights=(0, 0), dg=DG, env=None, img=None, mip1=None, mip3=None, flags=0, counter=False,
         bounds=BOUNDS, cascades=0, record=None, atlas=None, null_globals=False, ae=AE, scratch=SCRATCH, log_range=None):
    """One call. what: the hook's bits; size: the target's (and every full-resolution image's) extent; res: the globals'
    resolution (default: the same); lights: (point, spot) counts; img: {image: overrides of data (an offset), width, height,
    pitch, format}; mip1 / mip3: an extent, or True for the halved / eighth extent; cascades: the record's count (0: none);
    record: overrides of the record's fields; atlas: the shadow image's extent in a cascaded call."""
    return dict(what=what, size=size, res=res or size, lights=lights, dg=dg, env=env or {}, img=img or {}, mip1=mip1, mip3=mip3,
                flags=flags, counter=counter, bounds=bounds, cascades=cascades, record=record or {}, atlas=atlas,
                null_globals=null_globals, ae=ae, scratch=scratch, log_range=log_range)


FUSED = HIST            # the render graph's call: the fold is a pass of its own
ENTRY_HIST = HIST | FOLD
LIGHTS = ((0, 0), (3, 0), (0, 2), (3, 2))
SIZES = ((64, 36), (98, 56), (97, 55))
BAD = lambda name, **kw: call(img={name: kw})
NAN = float("nan")

CASES = {
    # the six entry points at the three extents, without and with lights
    "soc_composition": [call(size=s, lights=l) for s in SIZES for l in LIGHTS],
    "soc_composition_luminance_histogram": [call(ENTRY_HIST, size=s, lights=l) for s in SIZES for l in LIGHTS],
    "soc_composition_bounded": [call(BOUNDED, size=s, lights=l, flags=f, counter=c) for s in SIZES for l in ((0, 0), (3, 2))
                                for f in (0, 1) for c in (False, True)],
    "soc_composition_luminance_histogram_bounded": [call(ENTRY_HIST | BOUNDED, size=s, lights=l, flags=f, counter=c) for s in SIZES
                                                    for l in ((0, 0), (3, 2)) for f in (0, 1) for c in (False, True)],
    "soc_composition_cascaded": [call(CASCADED, size=s, lights=l, cascades=n) for s in SIZES for l in ((0, 0), (3, 2))
                                 for n in (1, 2, 3, 4)],
    "soc_composition_luminance_histogram_cascaded": [call(ENTRY_HIST | CASCADED, size=s, lights=l, cascades=n) for s in SIZES
                                                     for l in ((0, 0), (3, 2)) for n in (1, 2, 3, 4)],
    # the render graph's call: no fold, sky_external, the in-kernel bloom, the zero cells, bounds, cascades
    "internal": [call(FUSED, lights=l) for l in LIGHTS] + [call(FUSED | SKY_EXTERNAL, lights=l) for l in LIGHTS]
                + [call(FUSED | SKY_EXTERNAL, size=(64, 48), lights=l, mip1=m1, mip3=m3) for l in LIGHTS
                   for m1, m3 in ((True, None), (None, True), (True, True))]
                + [call(FUSED | BOUNDED, size=(64, 48), lights=l, flags=f, mip1=m1, mip3=m3) for l in ((0, 0), (3, 2)) for f in (0, 1)
                   for m1, m3 in ((None, None), (True, None), (None, True), (True, True))]
                + [call(FUSED | SKY_EXTERNAL | CASCADED, lights=l, cascades=n) for l in ((0, 0), (3, 2)) for n in (1, 4)]
                # a frame without lights has nothing to bound: the counter is no error beside the renderer-only forms
                + [call(FUSED | BOUNDED, size=(64, 48), counter=True, mip1=True, mip3=True)]
                # the counter on an accepted frame with lights, the fold off
                + [call(FUSED | BOUNDED, lights=(3, 2), flags=f, counter=True) for f in (0, 1)],
    "light_counts": [call(w, lights=l) for w in (0, ENTRY_HIST) for l in ((128, 0), (129, 0), (0, 128), (0, 129), (1000, 1000))],
    "extents": [call(w, size=s, cascades=2 if w & CASCADED else 0) for w in (0, ENTRY_HIST, ENTRY_HIST | CASCADED) for s in ((8192, 16), (8194, 16), (16, 8192), (16, 8194))]
               + [call(w, size=(64, 36), res=r, cascades=2 if w & CASCADED else 0) for w in (0, ENTRY_HIST, ENTRY_HIST | BOUNDED, ENTRY_HIST | CASCADED)
                  for r in ((128, 72), (64, 72))]
               + [call(w, img={n: dict(width=32, height=18)}) for w in (0, ENTRY_HIST) for n in IMAGES[1:]],
    "alignment": [call(w, img=i) for w in (0, ENTRY_HIST, BOUNDED) for i in (
        dict(target=dict(data=8)), dict(target=dict(pitch=64 * 8 + 8)), dict(albedo=dict(data=8)), dict(emissive=dict(pitch=64 * 8 + 8)),
        dict(normal=dict(data=8)), dict(depth=dict(data=4)), dict(depth=dict(pitch=64 * 4 + 4)), dict(clouds=dict(data=4)),
        dict(clouds=dict(pitch=64 * 4 + 4)), dict(ssao=dict(data=1, pitch=33)))],
    "knobs": [call(w, lights=l, env=e, mip1=m, cascades=2 if w & CASCADED else 0) for e in (dict(SOC_COMP_NT="0"), dict(SOC_COMP_AOP="0"),
                                                          dict(SOC_COMP_NT="0", SOC_COMP_AOP="0"), dict(SOC_BLOOM_ZERO_SKIP="0"))
              for w, m in ((0, None), (ENTRY_HIST, None), (FUSED, True), (CASCADED, None), (ENTRY_HIST | CASCADED, None))
              for l in ((0, 0), (3, 2))],
    "sky_compose": [call(SKY_COMPOSE, size=s) for s in SIZES]
                   + [call(SKY_COMPOSE, env=dict(SOC_SKY_COMPOSE_PAIR_LOAD="0")), call(SKY_COMPOSE, img=dict(clouds=dict(data=4))),
                      call(SKY_COMPOSE, img=dict(clouds=dict(pitch=64 * 4 + 4))), call(SKY_COMPOSE, log_range=(-3.0, -3.0)),
                      call(SKY_COMPOSE, null_globals=True), call(SKY_COMPOSE, scratch=None),
                      call(SKY_COMPOSE, img=dict(target=dict(format=RGBA8))), call(SKY_COMPOSE, img=dict(depth=dict(format=RGBA8))),
                      call(SKY_COMPOSE, img=dict(clouds=dict(format=R8)))],
    "histogram_range": [call(ENTRY_HIST, log_range=r) for r in ((-10.0, 20.0), (-3.0, -3.0), (0.0, 1e-3), (5.0, -5.0))],
    "rejections": [call(null_globals=True), call(ENTRY_HIST, null_globals=True), call(ENTRY_HIST, ae=None), call(ENTRY_HIST, scratch=None)]
                  + [BAD(n, format=D32F if FORMATS[n] != D32F else RGBA16F) for n in IMAGES]
                  + [BAD("target", data=-BASE["target"]), BAD("albedo", width=0), BAD("depth", pitch=64 * 4 - 4)]
                  + [call(lights=(1, 0), dg=None), call(ENTRY_HIST, lights=(0, 1), dg=None),
                     call(BOUNDED, bounds=None), call(BOUNDED, flags=2), call(ENTRY_HIST | BOUNDED, flags=3),
                     call(BOUNDED, lights=(1, 0), dg=None, bounds=None),
                     call(FUSED | BOUNDED, size=(64, 48), lights=(3, 2), counter=True, mip1=True),
                     call(FUSED | BOUNDED, size=(64, 48), lights=(3, 2), counter=True, mip3=True),
                     call(FUSED | CASCADED | BOUNDED, cascades=2), call(FUSED | CASCADED, cascades=2, mip1=True),
                     call(FUSED | CASCADED, cascades=2, mip3=True), call(CASCADED), call(CASCADED, cascades=2, record=dict(count=0)),
                     call(CASCADED, cascades=2, record=dict(count=5)), call(CASCADED, cascades=2, record=dict(map_size=1)),
                     call(CASCADED, cascades=2, record=dict(map_size=16385)), call(CASCADED, cascades=2, record=dict(pv=(1, 5, NAN))),
                     call(CASCADED, cascades=2, record=dict(ef=(1, math.inf))), call(CASCADED, cascades=3, record=dict(split=(0, NAN))),
                     call(CASCADED, cascades=3, record=dict(split=(1, 0.5))), call(CASCADED, cascades=2, img=dict(shadow=dict(format=RGBA16F))),
                     call(CASCADED, cascades=2, atlas=(SHADOW, SHADOW)), call(CASCADED, cascades=2, atlas=(2 * SHADOW, 2 * SHADOW)),
                     call(SKY_EXTERNAL), call(FUSED, mip1=True, img=dict(target=dict(data=8))),
                     call(FUSED, mip3=True, size=(97, 55)), call(FUSED | SKY_EXTERNAL, res=(128, 72)),
                     call(FUSED | SKY_EXTERNAL, mip1=True, mip3=True, res=(128, 72)), call(mip1=True), call(mip3=True),
                     call(FUSED, mip1=(32, 19)), call(FUSED, mip1=(31, 18)), call(FUSED, size=(64, 48), mip3=(8, 5)), call(FUSED, size=(64, 48), mip3=(9, 6)),
                     call(FUSED, mip1=(32, 18, D32F)), call(FUSED, mip3=(8, 4, RGBA8))],
}


def run_case(soc, name, setenv, delenv):
    """[(return code, error message, text)] of the case's calls, in order."""
    lib = soc.lib()
    out = []
    for c in CASES[name]:
        for k, v in c["env"].items():
            setenv(k, v)
        lib.soc_tuning_reload()
        (w, h), (gw, gh) = c["size"], c["res"]
        g = soc.globals_defaults(gw, gh)
        soc.frame_update(g, soc.make_camera((-14.0, 2.2, 0.3), (0.0, -0.42, 0.0)), gw, gh, 0.016, C.c_uint32(0))
        g.point_light_count, g.spot_light_count = c["lights"]
        if c["log_range"]:
            g.log_min_luminance, g.log_max_luminance = c["log_range"]
        n = c["cascades"]
        images = (soc.SocImg * 8)()
        for i, nm in enumerate(IMAGES):
            fmt = FORMATS[nm]
            ew, eh = ((w + 1) // 2, (h + 1) // 2) if nm == "ssao" else (SHADOW, SHADOW * max(n, 1)) if nm == "shadow" else (w, h)
            if nm == "shadow" and c["atlas"]:
                ew, eh = c["atlas"]
            o = c["img"].get(nm, {})
            ew, eh, fmt = o.get("width", ew), o.get("height", eh), o.get("format", fmt)
            images[i] = soc.SocImg(BASE[nm] + o.get("data", 0) or None, ew, eh, o.get("pitch", ew * BPP[fmt]), fmt)

        def mip(spec, base, div):
            if spec is None:
                return None
            mw, mh, fmt = (w // div, h // div, RGBA16F) if spec is True else (tuple(spec) + (RGBA16F,))[:3]
            return C.pointer(soc.SocImg(base, mw, mh, mw * BPP[fmt], fmt))
        rec = None
        if n:
            rec = _abi.SunCascades()
            rec.count, rec.map_size = n, SHADOW
            for k in range(4):
                for i in range(16):
                    rec.projection_view[k][i] = 0.01 * (1 + k) * (1 + i % 5) * (-1) ** i
                rec.split_depth[k] = 0.9 + 0.03 * k
                rec.exponential_factor[k] = -200.0 * (k + 1)
            r = c["record"]
            rec.count, rec.map_size = r.get("count", n), r.get("map_size", SHADOW)
            if "pv" in r:
                rec.projection_view[r["pv"][0]][r["pv"][1]] = r["pv"][2]
            if "ef" in r:
                rec.exponential_factor[r["ef"][0]] = r["ef"][1]
            if "split" in r:
                rec.split_depth[r["split"][0]] = r["split"][1]
        buf = C.create_string_buffer(4096)
        got = lib.soc_debug_plan_composition(None if c["null_globals"] else C.byref(g), c["dg"], images, c["what"], c["ae"],
                                             c["scratch"], mip(c["mip1"], MIP1, 2), mip(c["mip3"], MIP3, 8), c["bounds"], c["flags"],
                                             COUNTER if c["counter"] else None, C.byref(rec) if rec else None, buf, len(buf))
        assert got < len(buf)
        text = buf.value.decode() if got >= 0 else ""
        assert got < 0 or got == len(text)
        out.append((min(got, 0), lib.soc_last_error_string().decode() if got < 0 else "", text))
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
    assert {k: len(v) for k, v in golden["cases"].items()} == {k: len(v) for k, v in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_plans_are_the_recorded_ones(soc, golden, monkeypatch, name):
    got = run_case(soc, name, monkeypatch.setenv, monkeypatch.delenv)
    want = [(rc, msg, "".join(golden["lines"][i] for i in idx)) for rc, msg, idx in golden["cases"][name]]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, k, CASES[name][k])


def test_recorded_plans_show_what_the_cases_are_about(golden):
    """The fixture itself: the properties the cases were chosen for are in the recorded texts."""
    def steps(name, k):
        rc, msg, idx = golden["cases"][name][k]
        return rc, msg, [golden["lines"][i].rstrip("\n").split("\t") for i in idx]
    def kernels(name, k):
        return [(s[1], s[2]) for s in steps(name, k)[2] if s[0] == "kernel"]
    every = [(n, k) for n in CASES for k in range(len(CASES[n]))]
    seen = {kn for n, k in every for kn in kernels(n, k)}
    # every one of the 37 kernels is reached by some case
    assert len([k for k in seen if k[0] == "composition_pair"]) == 31 and len(seen) == 37
    # the knob rules: the lights forms are nt = 0, a cascaded or in-kernel-bloom form without lights is nt = 7 whatever the knobs
    for name, form in seen:
        if name == "composition_pair":
            f = dict(kv.split("=") for kv in form.split(" "))
            assert f["nt"] == "0" if f["lights"] == "1" else f["nt"] in ("0", "3", "7")
            if f["lights"] == "0" and (f["cs"] == "1" or f["bl"] == "1"):
                assert f["nt"] == "7"
    knob_forms = {(tuple(sorted(CASES["knobs"][k]["env"].items())), kn[1].split(" ")[2]) for k in range(len(CASES["knobs"]))
                  for kn in kernels("knobs", k) if kn[0] == "composition_pair" and " lights=0 " in kn[1] and " bl=0 " in kn[1]
                  and kn[1].endswith("cs=0")}
    assert ((("SOC_COMP_NT", "0"),), "nt=0") in knob_forms and ((("SOC_COMP_AOP", "0"),), "nt=3") in knob_forms
    assert ((("SOC_BLOOM_ZERO_SKIP", "0"),), "nt=7") in knob_forms
    # 97x55 is off the pair path: the generic kernel, and a histogram call is followed by the histogram pass
    assert kernels("soc_composition", 8) == [("composition_generic", "-")]
    assert steps("soc_composition_luminance_histogram", 8)[2][-1] == ["pass", "generate_luminance_histogram"]
    # on the pair path at another resolution than the globals': the pair kernel without the histogram, then the pass
    rc, _, st = steps("extents", 14)
    assert rc == 0 and " hist=0" in " " + st[1][2] and st[1][1] == "composition_pair" and st[-1][0] == "pass"
    # the entry points fold, the render graph's call does not
    assert ("histogram_fold", "-") in kernels("soc_composition_luminance_histogram", 0)
    assert ("histogram_fold", "-") not in kernels("internal", 0)
    # ... also with the counter on a frame with lights (lb = 5 without, 7 with the cull)
    n = len(CASES["internal"])
    assert [kernels("internal", k) for k in (n - 2, n - 1)] == [
        [("composition_pair", "hist=1 lights=1 nt=0 bl=0 sp=0 lb=%d cs=0" % lb)] for lb in (5, 7)]
    assert all(steps("internal", k)[2][1][-1] == "counter=1" for k in (n - 2, n - 1))
    # every rejection is one, and the three errors after a failed fusion are among them
    assert all(steps("rejections", k)[0] < 0 for k in range(len(CASES["rejections"])))
    msgs = {steps("rejections", k)[1] for k in range(len(CASES["rejections"]))}
    for m in ("composition: the bloom's zero cells need the pair path", "composition: the in-kernel bloom needs the pair path",
              "composition: sky_external needs the pair path"):
        assert m in msgs
