"""The wave-level culling predicates of the bounded lights (csrc/light_cull.hpp: sphere against box with a range, outer
cone against the box's bounding sphere) are conservative by their stated slacks: tools/check_light_cull.cpp checks 1.2 M
seeded (box, light) cases, a quarter of them grazing a corner, an edge or a face within 1e-4, against float64 geometry
at 68 sampled points of the box, and that lights placed far away are in fact culled (~2 s)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_light_cull_conservative(tmp_path):
    exe = str(tmp_path / "check_light_cull")
    subprocess.run(["g++", "-O2", os.path.join(ROOT, "tools", "check_light_cull.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    m = re.search(r"cases (\d+): grazing (\d+), far range (\d+), far cone (\d+), apex inside (\d+), box behind (\d+); "
                  r"range culled (\d+), cone culled (\d+); failures 0", r.stdout)
    assert m, r.stdout
    cases, grazing, far_r, far_c, inside, behind, culled_r, culled_c = map(int, m.groups())
    assert cases >= 1_000_000 and grazing * 4 == cases
    assert min(far_r, far_c, inside, behind) > 50_000
    # neither predicate is vacuous: far lights alone are an eighth of the cases
    assert culled_r > far_r and culled_c > far_c
