"""The microbenchmarks under tools/ubench are cited as evidence in DESIGN.md (issue model, residency, range check): keep them compiling."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("name", ["mfma_issue", "residency", "soffset_probe"])
def test_microbenchmark_cross_compiles_for_gfx950(name, tmp_path):
    src = os.path.join(ROOT, "tools", "ubench", name + ".hip")
    out = tmp_path / (name + ".o")
    r = subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-Wno-unused-value", "-c", src, "-o", str(out)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.stat().st_size > 0


def test_the_functions_of_the_five_headers_are_pairwise_disjoint():
    """The main library's header and every entry of ``build.EXTENSIONS``: a function is declared by one header and exported by one library."""
    from _surface import header
    from driving_dirty_amd import build
    assert list(build.EXTENSIONS) == ["augment", "tta", "ema", "rm_loss"]
    headers = [build.HEADER] + [e.header for e in build.EXTENSIONS.values()]
    assert len(set(headers)) == 5 and all(os.path.dirname(h) == os.path.join(ROOT, "include") for h in headers)
    names = {h: set(header(os.path.basename(h))[0]) for h in headers}
    assert all(names.values())
    for i, a in enumerate(headers):
        for b in headers[i + 1:]:
            assert not names[a] & names[b], (a, b, names[a] & names[b])
    for name, e in build.EXTENSIONS.items():
        assert e.name == name and e.header in e.headers and build.HEADER in e.headers and e.what
        assert os.path.dirname(e.lib) == build.CSRC and all(os.path.exists(os.path.join(build.CSRC, s)) for s in e.sources)


def test_the_build_issues_the_commands_of_the_table(monkeypatch):
    """``build._run`` records instead of running: nothing when nothing is stale; an extension is one compile per source with the main
    library's flags and one link against it; the main library hands EXTRA_FLAGS to the file they name and to no other."""
    from driving_dirty_amd import build
    assert not build.needs_build(), "build the HIP libraries first (python __graft_entry__.py)"
    commands = []
    monkeypatch.setattr(build, "_run", lambda cmd, verbose: commands.append(cmd))
    assert build.build(verbose=False) == build.LIB and commands == []
    for name, e in build.EXTENSIONS.items():
        assert not build.extension_needs_build(name) and build.build_extension(name, verbose=False) == e.lib and commands == []
        assert build.build_extension(name, force=True, verbose=False) == e.lib
        *compiles, link = commands
        objs = [os.path.join(build.OBJ, os.path.splitext(s)[0] + ".o") for s in e.sources]
        assert sorted(compiles) == sorted([link[0]] + build.FLAGS + ["-c", os.path.join(build.CSRC, s), "-o", o] for s, o in zip(e.sources, objs))
        assert link[1:] == ["--offload-arch=gfx950", "-shared", "-fPIC", "-o", e.lib] + objs + ["-L" + build.CSRC, "-l:libdd_hotpath.so", "-Wl,-rpath,$ORIGIN"]
        del commands[:]
    assert build._build_main(force=True, verbose=False) == build.LIB
    *compiles, link = commands
    assert len(compiles) == len(build.SOURCES) and set(build.EXTRA_FLAGS) == {"adam_rankb.hip"}
    by_source = {os.path.basename(c[c.index("-c") + 1]): c for c in compiles}
    assert set(by_source) == set(build.SOURCES)
    for src, c in by_source.items():
        assert c[1:] == build.FLAGS + build.EXTRA_FLAGS.get(src, []) + ["-c", os.path.join(build.CSRC, src), "-o", os.path.join(build.OBJ, os.path.splitext(src)[0] + ".o")]
        assert ("-amdgpu-mfma-vgpr-form" in c) == (src == "adam_rankb.hip")
    assert link[1:] == ["--offload-arch=gfx950", "-shared", "-fPIC", "-o", build.LIB] + [os.path.join(build.OBJ, os.path.splitext(s)[0] + ".o") for s in build.SOURCES]
