#!/usr/bin/env python3
"""Host-side sanitizer pass over the C ABI (VERDICT r1 missing #3).

    python scripts/sanitize_host.py [--iters N] [--keep]

1. compiles the library's sources (momlevel_amd.csrc.build.SOURCES) with the HOST pass instrumented by
   AddressSanitizer + UndefinedBehaviorSanitizer (``-fsanitize=address,undefined
   -fno-gpu-sanitize``: the gfx950 device code is built as always and never instrumented -- GPU
   ASan is not available on this pool and is not used) into build/sanitize/libmomlevel_hip.so;
2. builds tests/native/abi_fuzz.cpp against it and runs it (fake pointers, GPU-less process only:
   every call ends in an MLX_E_* code or hipErrorNoDevice from the launch);
3. runs tests/test_abi.py in a python whose momlevel_amd binds the sanitized library
   (MOMLEVEL_AMD_LIB + LD_PRELOAD of the ASan runtime).
Any ASan/UBSan report is fatal.  Never run on a GPU box: the fuzzer refuses, exit code 77.
"""
import argparse
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build", "sanitize")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-gpu-sanitize",
       "-fno-omit-frame-pointer", "-g", "-O1"]


def hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def run(cmd, **kw):
    print("+", " ".join(cmd), flush=True)
    return subprocess.run(cmd, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20000)
    ap.add_argument("--skip-pytest", action="store_true")
    a = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    lib = os.path.join(OUT, "libmomlevel_hip.so")
    sys.path.insert(0, ROOT)
    from momlevel_amd.csrc import build  # the library's own source list: nothing to keep in step

    srcs = list(build.SOURCES)
    deps = list(build.DEPENDS) + [os.path.abspath(__file__)]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(map(os.path.getmtime, deps)):
        run([hipcc(), "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC", "-shared",
             "-std=c++17"] + SAN + srcs + ["-o", lib], check=True)
    exe = os.path.join(OUT, "abi_fuzz")
    run([hipcc(), "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__"] + SAN +
        [os.path.join(ROOT, "tests", "native", "abi_fuzz.cpp"), "-I/opt/rocm/include",
         "-L" + OUT, "-lmomlevel_hip", "-L/opt/rocm/lib", "-lamdhip64",
         "-Wl,-rpath," + OUT + ":/opt/rocm/lib", "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = run([exe, str(a.iters)], env=env)
    if r.returncode != 0:
        return r.returncode
    if not a.skip_pytest:
        rt = subprocess.run([os.path.join(os.path.dirname(os.path.realpath(hipcc())), "..", "lib",
                                          "llvm", "bin", "clang"),
                             "--print-file-name=libclang_rt.asan-x86_64.so"],
                            capture_output=True, text=True).stdout.strip()
        if not os.path.isabs(rt) or not os.path.exists(rt):
            rt = subprocess.run(["/opt/rocm/lib/llvm/bin/clang",
                                 "--print-file-name=libclang_rt.asan-x86_64.so"],
                                capture_output=True, text=True).stdout.strip()
        env2 = dict(env, MOMLEVEL_AMD_LIB=lib, LD_PRELOAD=rt, MOMLEVEL_AMD_SANITIZED="1")
        r = run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider",
                 os.path.join(ROOT, "tests", "test_abi.py")], env=env2, cwd=ROOT)
        if r.returncode != 0:
            return r.returncode
    print("sanitize_host OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
