"""The one C99 harness of the ABI tests: a C program that includes include/esn_hip.h is compiled as strict C99,
linked against the built libesn_hip.so and run (no GPU needed: the callers exercise host-only entry points and
argument checks)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_and_run(tmp_path, name, source, extra_link=()):
    """Write `source` to tmp_path/name.c, build it against the library, run it, assert both return codes; returns the
    CompletedProcess of the run.  `extra_link`: further link arguments, placed after -lesn_hip."""
    from esn_ofdm_mimo_amd import build
    libdir = os.path.dirname(build.build_library(verbose=False))
    src, exe = os.path.join(str(tmp_path), name + ".c"), os.path.join(str(tmp_path), name)
    with open(src, "w") as f:
        f.write(source)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src,
           "-o", exe, "-L", libdir, "-lesn_hip", *extra_link, "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    return r
