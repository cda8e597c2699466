"""tools/collapse_study.cpp REBUILD=bottom (the CPU study behind the walk-only tree): the tool builds,
and a tree whose subtrees of <= BOT_K leaves were rebuilt is still a tree over the same leaves -- the counted walk
finds the same hit for every ray and tests about as many triangles -- whatever BOT_K."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    d = tmp_path_factory.mktemp("collapse_study")
    exe = str(d / "collapse_study")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", os.path.join(REPO, "tools", "collapse_study.cpp"), "-o", exe],
                   check=True)
    subprocess.run([sys.executable, os.path.join(REPO, "tests", "collapse_study_inputs.py"), str(d / "in"), "3000", "2"],
                   check=True, capture_output=True)

    def run(**env):
        r = subprocess.run([exe, str(d / "in")], check=True, capture_output=True, text=True, env={**os.environ, **env})
        return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr
    return run


def test_bottom_rebuild_keeps_the_leaves_and_the_hits(study):
    base, _ = study()
    assert base["T"] == 3000 and base["rays"] > 1000
    for k, roots in (("2", None), ("64", None), ("512", None), ("3000", 1)):
        got, err = study(REBUILD="bottom", BOT_K=k)
        assert f"subtrees of <= {k} leaves rebuilt" in err
        if roots is not None:   # the whole tree is one subtree: the root keeps its id
            assert err.startswith(f"bottom: {roots} subtrees") and "2999 internal nodes" in err
        assert got["greedy"]["hits"] == base["greedy"]["hits"] and got["sah_opt"]["hits"] == base["sah_opt"]["hits"]
        assert abs(got["greedy"]["leaf_tests"] - base["greedy"]["leaf_tests"]) < 0.25 * base["greedy"]["leaf_tests"]
    assert study(REBUILD="bottom")[1].count("<= 512 leaves") == 1   # BOT_K's default
