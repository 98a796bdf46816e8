"""Tuning builds never replace the installed kernel library (CPU only; skipped without hipcc): ``make`` refuses EXTRA on
the default goal, tools/variant.sh builds ``tail_chain`` with -DTC_STAMPS (one extra export, lpf_tail_chain_set_stamps,
tells the variant from the product) into a library of its own under csrc/build/variants/, passes on the command's status
and time limit, does not run the command after a failed build, and LPF_HIP_LIB -- and nothing else -- decides which
library a process loads."""
import hashlib
import importlib.util
import os
import re
import subprocess
import sys

import pytest

from lpformer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("tail_isa", os.path.join(ROOT, "tools", "tail_isa.py"))
tail_isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tail_isa)

pytestmark = pytest.mark.skipif(tail_isa.find_hipcc() is None, reason="needs hipcc")
CSRC = os.path.join(ROOT, "lpformer_amd", "csrc")
RUNNER = os.path.join(ROOT, "tools", "variant.sh")
SETTER = "lpf_tail_chain_set_stamps"
BUILD_FAILED = 96      # tools/variant.sh's own status for a failed build (its header)
STAMPED = ["-s", "tail_chain", "-x", "-DTC_STAMPS"]


def clean_env(**more):
    """The environment of a child: no variant selected, no runner switch, the compiler this module found."""
    env = {k: v for k, v in os.environ.items() if k not in ("LPF_HIP_LIB", "VARIANT_BUILD_ONLY", "EXTRA", "VARIANT")}
    env["HIPCC"] = tail_isa.find_hipcc()
    env.update(more)
    return env


def sha256(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def exported(path):
    """The defined dynamic symbols lpf_* of a shared object."""
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.split()[-1].startswith("lpf_")}


def runner(*args, **env):
    return subprocess.run([RUNNER, *args], env=clean_env(**env), cwd=ROOT, capture_output=True, text=True, timeout=600)


def named_library(p):
    """The library path of the runner's one line about what the command runs on."""
    lines = [l for l in p.stderr.splitlines() if l.startswith("[variant] flags=")]
    assert len(lines) == 1, p.stderr
    return re.search(r" lib=(.+)$", lines[0]).group(1)


def build_stamped_variant():
    """Default ``make`` (a no-op when built), then the -DTC_STAMPS variant of tail_chain through the runner:
    (SHA-256 of the installed library before the variant was built, the variant library's path)."""
    subprocess.run(["make", "-C", CSRC, "-j8"], env=clean_env(), check=True, capture_output=True)
    before = sha256(_lib.INSTALLED_HIP_LIB_PATH)
    p = runner("-n", *STAMPED, "-t", "60", "--", "true")
    assert p.returncode == 0, p.stderr
    return before, named_library(p)


@pytest.fixture(scope="module")
def built():
    return build_stamped_variant()


def test_make_refuses_extra_on_the_default_goal(built):
    p = subprocess.run(["make", "-C", CSRC, "EXTRA=-DTC_STAMPS"], env=clean_env(), capture_output=True, text=True)
    assert p.returncode != 0 and "variant" in p.stderr, p.stderr
    assert sha256(_lib.INSTALLED_HIP_LIB_PATH) == built[0]


def test_variant_is_a_library_of_its_own(built):
    before, lib = built
    assert os.path.isfile(lib)
    assert os.path.commonpath([lib, os.path.join(CSRC, "build", "variants")]) == os.path.join(CSRC, "build", "variants")
    assert exported(lib) == set(_lib.HIP_PROTOTYPES) | {SETTER}
    assert SETTER not in exported(_lib.INSTALLED_HIP_LIB_PATH)
    assert sha256(_lib.INSTALLED_HIP_LIB_PATH) == before


def test_same_flags_are_not_rebuilt(built):
    obj = os.path.join(os.path.dirname(built[1]), "tail_chain.o")
    src = os.path.join(CSRC, "tail_chain.hip")
    mtime, src_mtime = os.stat(obj).st_mtime_ns, os.stat(src).st_mtime_ns
    p = runner("-n", "-s", "tail_chain", "-x", "-DTC_STAMPS ", "-t", "60", "--", "true")   # (as tail_stamps.sh "" passes it)
    assert p.returncode == 0 and named_library(p) == built[1], p.stderr
    assert os.stat(obj).st_mtime_ns == mtime
    assert os.stat(src).st_mtime_ns == src_mtime      # (no source is ever touched to force a build)


def test_failed_build_does_not_run_the_command(built, tmp_path):
    marker = tmp_path / "ran"
    p = runner("-s", "tail_chain", "-x", f"-include {tmp_path}/no_such_header.h", "-t", "60", "--", "touch", str(marker))
    assert p.returncode == BUILD_FAILED, (p.returncode, p.stderr)
    assert "no_such_header.h" in p.stderr      # the end of the build log
    assert not marker.exists()
    assert sha256(_lib.INSTALLED_HIP_LIB_PATH) == built[0]


def test_build_only_switch_does_not_run_the_command(built, tmp_path):
    marker = tmp_path / "ran"
    p = runner(*STAMPED, "-t", "60", "--", "touch", str(marker), VARIANT_BUILD_ONLY="1")
    assert p.returncode == 0 and named_library(p) == built[1] and not marker.exists(), p.stderr


def test_command_status_and_time_limit_are_passed_on(built):
    assert runner(*STAMPED, "-t", "60", "--", "sh", "-c", "exit 7").returncode == 7
    assert runner("-t", "60", "--", "sh", "-c", "exit 7").returncode == 7
    assert runner("-t", "1", "--", "sleep", "5").returncode == 124
    assert runner("--", "true").returncode == 64                                 # no -t: usage
    assert runner("-x", "-DTC_STAMPS", "-t", "60", "--", "true").returncode == 64  # flags without sources: usage


def test_command_sees_the_library_it_was_built_for(built):
    show = ["sh", "-c", 'echo "lib=${LPF_HIP_LIB-unset}"']
    assert runner(*STAMPED, "-t", "60", "--", *show).stdout == f"lib={built[1]}\n"
    p = runner("-s", "tail_chain", "-x", "", "-t", "60", "--", *show, LPF_HIP_LIB=built[1])
    assert p.stdout == "lib=unset\n" and named_library(p) == _lib.INSTALLED_HIP_LIB_PATH, (p.stdout, p.stderr)
    assert sha256(_lib.INSTALLED_HIP_LIB_PATH) == built[0]


def _child(code, lib):
    return subprocess.run([sys.executable, "-c", code], env=clean_env(LPF_HIP_LIB=lib), cwd=ROOT, capture_output=True,
                          text=True, timeout=120)


def test_lpf_hip_lib_selects_the_library(built, tmp_path):
    p = _child("from lpformer_amd import _lib\n"
               "print(_lib.HIP_LIB_PATH)\n"
               "lib = _lib.hip()\n"       # binds the header's prototypes, checks the ABI version; needs no GPU
               f"print(hasattr(lib, '{SETTER}'), lib.lpf_abi_version() == _lib.ABI_VERSION)\n", built[1])
    assert p.returncode == 0 and p.stdout.split() == [built[1], "True", "True"], (p.stdout, p.stderr)
    missing = str(tmp_path / "liblpformer_hip.so")
    p = _child("from lpformer_amd import _lib\n"
               "print(_lib.HIP_LIB_PATH)\n"
               "try:\n"
               "    _lib.hip()\n"
               "except _lib.LpfError as e:\n"
               "    print('LpfError:', e)\n", missing)
    out = p.stdout.splitlines()
    assert p.returncode == 0 and out[0] == missing and out[1].startswith("LpfError:"), (p.stdout, p.stderr)
    assert "LPF_HIP_LIB" in out[1] and missing in out[1]


def test_the_suite_runs_on_the_installed_library():
    assert "LPF_HIP_LIB" not in os.environ
    assert _lib.HIP_LIB_PATH == _lib.INSTALLED_HIP_LIB_PATH
    assert os.path.dirname(_lib.INSTALLED_HIP_LIB_PATH) == os.path.join(ROOT, "lpformer_amd")
