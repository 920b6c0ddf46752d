"""Builds libohs_hip.so (HIP kernels + C ABI), libohs_scene.so (the same objects + the ohs_scene_* entries), libohs_scene2.so (the
same objects + the ohs_scene2_* entries), libohs_scene3.so (the same objects + the ohs_scene3_* entries), libohs_lookup.so (its
own two objects and nothing of the product's), libohs_lookup3.so (likewise its own two), libohs_lookup3p.so (likewise),
libohs_tracked.so (the product's objects + lookup3p_kernels.o + its own two units, the ohs_tracked_* entries), libohs_delay.so
(its own two objects and nothing of the product's, the ohs_delay_* entries) and libohs_delay2.so (likewise its own two, the
ohs_delay2_* entries) for gfx950, in-tree.

    python -m open_headstage_amd.build [--force]

hipcc cross-compiles without a GPU.  eq_kernels.hip is compiled with
-ffp-contract=off: the biquad recurrence must round every product and sum
separately to be bit-exact with the reference's arithmetic.

Staleness is decided by CONTENT (sha256 of each unit's source, every header / .inc it may include, its
flags and this file), recorded in libohs_hip.stamp next to the library -- not by mtimes, which a
snapshot copy to the GPU box does not keep.  `is_current()` lets the test session refuse a library
that does not match the sources it is about to test.
"""
from __future__ import annotations

import hashlib
import json
import os
import shutil
import subprocess
import sys

# (TAG / EXPERIMENTS below read sys.argv: `python -m open_headstage_amd.build --experiments`)
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
# Experiment variants: OHS_BUILD_TAG=name OHS_EXTRA_DEFS="-DFOO=1 ..." builds libohs_hip_name.so beside the
# product library (objects under build/name/); OHS_LIB=<path> makes _ffi.py load it.  Not used in production.
#
# Two libraries come out of this file:
#   libohs_hip.so       the PRODUCT: reads no environment variable, no experiment variant compiled in (csrc/experiments.h)
#   libohs_hip_exp.so   the EXPERIMENTS build (-DOHS_EXPERIMENTS): the same code plus the OHS_* environment knobs, the debug
#                       entry points (ohs_debug_set_tuning ...) and round 2's EQ kernel; `--experiments`, or
#                       OHS_BUILD_TAG=exp.  Other tags (OHS_BUILD_TAG=name OHS_EXTRA_DEFS="-DFOO") are variants OF the
#                       experiments build: every tagged library is compiled with -DOHS_EXPERIMENTS.
TAG = os.environ.get("OHS_BUILD_TAG", "")
if "--experiments" in sys.argv and not TAG:
    TAG = "exp"
EXPERIMENTS = bool(TAG)
EXTRA_DEFS = os.environ.get("OHS_EXTRA_DEFS", "").split() + (["-DOHS_EXPERIMENTS=1"] if EXPERIMENTS else [])
OBJ = os.path.join(HERE, "build", TAG) if TAG else os.path.join(HERE, "build")
LIB = os.path.join(HERE, f"libohs_hip_{TAG}.so" if TAG else "libohs_hip.so")
STAMP = os.path.join(HERE, f"libohs_hip_{TAG}.stamp" if TAG else "libohs_hip.stamp")
# per-kernel register / scratch / LDS figures as hipcc reports them (-Rpass-analysis=kernel-resource-usage), written
# next to the library at build time: DESIGN.md quotes them and tests/test_cpu_host_logic.py holds k_eq_ring to its
# 32-VGPR budget with them
RESOURCES = os.path.join(HERE, f"libohs_hip_{TAG}.resources.json" if TAG else "libohs_hip.resources.json")
# The SCENE library (include/ohs_scene.h): the product's object files plus api_scene.o, exporting ohs_scene_* and nothing else
# (csrc/scene_exports.map).  Untagged build only; libohs_hip.so links without api_scene.o.
SCENE_LIB = os.path.join(HERE, "libohs_scene.so")
SCENE_UNIT = ("api_scene.hip", [])
# The second SCENE library (include/ohs_scene2.h): the product's object files plus api_scene2.o, exporting ohs_scene2_* and nothing
# else (csrc/scene2_exports.map).  Untagged build only.
SCENE2_LIB = os.path.join(HERE, "libohs_scene2.so")
SCENE2_UNIT = ("api_scene2.hip", [])
# The third SCENE library (include/ohs_scene3.h): the product's object files plus api_scene3.o, exporting ohs_scene3_* and nothing
# else (csrc/scene3_exports.map).  Untagged build only.
SCENE3_LIB = os.path.join(HERE, "libohs_scene3.so")
SCENE3_UNIT = ("api_scene3.hip", [])
# The LOOKUP library (include/ohs_lookup.h): direction indices and weights for the scene calls, found on the device.  Its own two
# units and none of the product's objects, exporting ohs_lookup_* and nothing else (csrc/lookup_exports.map).  Untagged build only.
# Every operation of the search rounds by itself (-ffp-contract=off): the answers are tests/lookup_model.py's bits.
LOOKUP_LIB = os.path.join(HERE, "libohs_lookup.so")
LOOKUP_UNITS = [("lookup_kernels.hip", ["-ffp-contract=off"]), ("api_lookup.hip", ["-ffp-contract=off"])]
LOOKUP_HEADERS = ("lookup_body.hpp", "lookup_internal.h")
# The second LOOKUP library (include/ohs_lookup3.h): the three indices and two weights per object that libohs_scene3.so renders, found
# over a triangle mesh on the device.  Its own two units again, none of the product's objects and none of libohs_lookup.so's, exporting
# ohs_lookup3_* and nothing else (csrc/lookup3_exports.map).  Untagged build only.  -ffp-contract=off: the answers are
# scene3.triangle_directions' bits (tests/lookup3_model.py).  The units include lookup_body.hpp for lookup_pose.
LOOKUP3_LIB = os.path.join(HERE, "libohs_lookup3.so")
LOOKUP3_UNITS = [("lookup3_kernels.hip", ["-ffp-contract=off"]), ("api_lookup3.hip", ["-ffp-contract=off"])]
LOOKUP3_HEADERS = ("lookup3_body.hpp", "lookup3_internal.h")
# The third LOOKUP library (include/ohs_lookup3p.h): libohs_lookup3.so's rows with the walk pruned by a grid over the sphere, bit for
# bit.  Its own two units once more, none of the product's objects and none of the other lookup libraries', exporting ohs_lookup3p_*
# and nothing else (csrc/lookup3p_exports.map).  Untagged build only.  -ffp-contract=off as above.  The units include lookup3_body.hpp
# and lookup_body.hpp as they are.
LOOKUP3P_LIB = os.path.join(HERE, "libohs_lookup3p.so")
LOOKUP3P_UNITS = [("lookup3p_kernels.hip", ["-ffp-contract=off"]), ("api_lookup3p.hip", ["-ffp-contract=off"])]
LOOKUP3P_HEADERS = ("lookup3p_body.hpp", "lookup3p_internal.h")
# The TRACKED library (include/ohs_tracked.h): sources and poses in, two ears out, the rows found, sealed and rendered on the device
# on one stream.  The product's object files, as libohs_scene3.so links them, plus lookup3p_kernels.o and two units of its own,
# exporting ohs_tracked_* and nothing else (csrc/tracked_exports.map).  Untagged build only.  api_tracked.hip builds the mesh's
# inverses and index on the host as api_lookup3p.hip does: -ffp-contract=off, the same bits.
TRACKED_LIB = os.path.join(HERE, "libohs_tracked.so")
TRACKED_UNITS = [("scene_rows_kernels.hip", []), ("api_tracked.hip", ["-ffp-contract=off"])]
TRACKED_HEADERS = ("scene_rows_body.hpp", "scene_rows_internal.h")
# The DELAY library (include/ohs_delay.h): per-object propagation delay and gain in front of the scene calls, device to device on the
# caller's stream (k_object_delay).  Its own two units and none of the product's objects, as the lookup libraries are built, exporting
# ohs_delay_* and nothing else (csrc/delay_exports.map).  Untagged build only.  -ffp-contract=off: every operation of the header's
# arithmetic rounds by itself, the answers are tests/delay_model.py's bits.
DELAY_LIB = os.path.join(HERE, "libohs_delay.so")
DELAY_UNITS = [("delay_kernels.hip", ["-ffp-contract=off"]), ("api_delay.hip", ["-ffp-contract=off"])]
DELAY_HEADERS = ("delay_body.hpp", "delay_internal.h")
# The second DELAY library (include/ohs_delay2.h): the same stage with a distance-dependent symmetric FIR fused into it
# (k_object_delay2).  Its own two units again, none of the product's objects and none of libohs_delay.so's, exporting ohs_delay2_* and
# nothing else (csrc/delay2_exports.map).  Untagged build only.  -ffp-contract=off: the answers are tests/delay2_model.py's bits, and
# its unfiltered call has libohs_delay.so's.  The units include delay_body.hpp as it is.
DELAY2_LIB = os.path.join(HERE, "libohs_delay2.so")
DELAY2_UNITS = [("delay2_kernels.hip", ["-ffp-contract=off"]), ("api_delay2.hip", ["-ffp-contract=off"])]
DELAY2_HEADERS = ("delay2_body.hpp", "delay2_internal.h")
ARCH = "gfx950"


def _units():
    # (source, extra flags)
    return [
        # FFT kernels: no SLP vectoriser (see conv_mac_kernels.hip); no implicit FMA contraction -- the fused
        # operations are written out (wave_fft.hpp), so that every kernel inlining them rounds alike
        ("conv_kernels.hip", ["-fno-slp-vectorize", "-ffp-contract=off"]),
        ("conv_os_kernels.hip", ["-fno-slp-vectorize", "-ffp-contract=off"]),   # the overlap-save plan of the P = 1 path
        ("conv_lb_kernels.hip", ["-fno-slp-vectorize", "-ffp-contract=off"]),   # block 2048 / FFT 4096 for long impulse responses
        ("conv_xb_kernels.hip", ["-fno-slp-vectorize", "-ffp-contract=off"]),   # block 8192 / FFT 16384 in one kernel: their long out-of-place calls
        ("conv_objects_kernels.hip", ["-fno-slp-vectorize", "-ffp-contract=off"]),   # K moving sources per stream (libohs_scene.so reaches it)
        ("conv_objects_blend_kernels.hip", ["-fno-slp-vectorize", "-ffp-contract=off"]),   # ... between two directions each (libohs_scene2.so)
        ("conv_objects_blend3_kernels.hip", ["-fno-slp-vectorize", "-ffp-contract=off"]),  # ... inside a triangle of three (libohs_scene3.so)
        # (experiments builds only: OHS_MAC_TB / OHS_MAC_PI fix the MAC's register tile)
        ("conv_mac_kernels.hip", [f"-D{k}={os.environ[k]}" for k in ("OHS_MAC_TB", "OHS_MAC_PI")
                                  if EXPERIMENTS and k in os.environ]),
        ("eq_kernels.hip", ["-ffp-contract=off"]),
        ("api_core.hip", []), ("api_conv.hip", []), ("api_eq.hip", []), ("api_engine.hip", []), ("api_batch.hip", []),   # the C ABI (api_internal.h)
        ("sofa_reader.cpp", ["-x", "hip"]),     # host-only C++ (HDF5 subset reader), built by the same driver
        ("sofa_conditioning.cpp", ["-x", "hip"]),   # host-only C++ (libmysofa-style loudness / interpolation)
        ("autoeq_parser.cpp", ["-x", "hip"]),   # host-only C++ (AutoEQ CSV)
        ("node_batch.cpp", ["-x", "hip"]),      # host-only C++ (batch mode over the GPUs of a node; RCCL by dlopen)
        ("speakers.cpp", ["-x", "hip"]),        # host-only C++ (speaker angles -> four HRIRs off a SOFA handle)
        ("tuning.cpp", ["-x", "hip"]),          # host-only C++ (launch-plan constants; environment knobs in experiments builds)
        # host-only C++ (RBJ coefficient formulas + the musl restatement of sinf / cosf / powf: every operation rounds
        # by itself)
        ("biquad_coeffs.cpp", ["-x", "hip", "-ffp-contract=off"]),
    ]


COMMON = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function",
          "-Wno-unused-value", "-Wno-unused-result"]


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found")


def _deps(src: str) -> list[str]:
    deps = [os.path.join(CSRC, src)]
    if src in [u for u, _ in LOOKUP_UNITS]:             # (the lookup library includes its own headers and ohs_hip.h's status codes)
        deps += [os.path.join(CSRC, f) for f in LOOKUP_HEADERS]
        deps += [os.path.join(os.path.dirname(HERE), "include", f) for f in ("ohs_hip.h", "ohs_lookup.h")]
        return deps + [os.path.join(CSRC, "lookup_exports.map"), os.path.abspath(__file__)]
    if src in [u for u, _ in LOOKUP3_UNITS]:            # (likewise, and lookup_body.hpp for lookup_pose)
        deps += [os.path.join(CSRC, f) for f in LOOKUP3_HEADERS + ("lookup_body.hpp",)]
        deps += [os.path.join(os.path.dirname(HERE), "include", f) for f in ("ohs_hip.h", "ohs_lookup3.h")]
        return deps + [os.path.join(CSRC, "lookup3_exports.map"), os.path.abspath(__file__)]
    if src in [u for u, _ in LOOKUP3P_UNITS]:           # (likewise, and the two older bodies it includes)
        deps += [os.path.join(CSRC, f) for f in LOOKUP3P_HEADERS + ("lookup3_body.hpp", "lookup_body.hpp")]
        deps += [os.path.join(os.path.dirname(HERE), "include", f) for f in ("ohs_hip.h", "ohs_lookup3p.h")]
        return deps + [os.path.join(CSRC, "lookup3p_exports.map"), os.path.abspath(__file__)]
    if src in [u for u, _ in DELAY_UNITS]:              # (its own headers and ohs_hip.h's status codes, as the first lookup library)
        deps += [os.path.join(CSRC, f) for f in DELAY_HEADERS]
        deps += [os.path.join(os.path.dirname(HERE), "include", f) for f in ("ohs_hip.h", "ohs_delay.h")]
        return deps + [os.path.join(CSRC, "delay_exports.map"), os.path.abspath(__file__)]
    if src in [u for u, _ in DELAY2_UNITS]:             # (likewise, and the older body it includes)
        deps += [os.path.join(CSRC, f) for f in DELAY2_HEADERS + ("delay_body.hpp",)]
        deps += [os.path.join(os.path.dirname(HERE), "include", f) for f in ("ohs_hip.h", "ohs_delay2.h")]
        return deps + [os.path.join(CSRC, "delay2_exports.map"), os.path.abspath(__file__)]
    tracked = src in [u for u, _ in TRACKED_UNITS]      # (the product's headers, its own, and the pruned lookup's with the bodies it includes)
    deps += sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC)
                   if f.endswith((".h", ".hpp", ".inc")) and f not in LOOKUP_HEADERS + LOOKUP3_HEADERS + LOOKUP3P_HEADERS + TRACKED_HEADERS + DELAY_HEADERS +
                   DELAY2_HEADERS)
    if tracked:
        deps += [os.path.join(CSRC, f) for f in TRACKED_HEADERS + LOOKUP3P_HEADERS + ("lookup3_body.hpp", "lookup_body.hpp")]
    exp_dir = os.path.join(CSRC, "experiments")         # (included under -DOHS_EXPERIMENTS only)
    if os.path.isdir(exp_dir):
        deps += sorted(os.path.join(exp_dir, f) for f in os.listdir(exp_dir) if f.endswith((".h", ".hpp", ".inc")))
    deps.append(os.path.join(os.path.dirname(HERE), "include", "ohs_hip.h"))
    deps.append(os.path.join(CSRC, "exports.map"))
    if src == SCENE_UNIT[0]:
        deps.append(os.path.join(os.path.dirname(HERE), "include", "ohs_scene.h"))
        deps.append(os.path.join(CSRC, "scene_exports.map"))
    if src == SCENE2_UNIT[0]:
        deps.append(os.path.join(os.path.dirname(HERE), "include", "ohs_scene2.h"))
        deps.append(os.path.join(CSRC, "scene2_exports.map"))
    if src == SCENE3_UNIT[0]:
        deps.append(os.path.join(os.path.dirname(HERE), "include", "ohs_scene3.h"))
        deps.append(os.path.join(CSRC, "scene3_exports.map"))
    if tracked:
        deps.append(os.path.join(os.path.dirname(HERE), "include", "ohs_tracked.h"))
        deps.append(os.path.join(CSRC, "tracked_exports.map"))
    deps.append(os.path.abspath(__file__))
    return deps


def _unit_hash(src: str, extra: list[str]) -> str:
    h = hashlib.sha256()
    h.update(" ".join(COMMON + extra + EXTRA_DEFS).encode())
    for d in _deps(src):
        h.update(os.path.basename(d).encode())
        with open(d, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def _all_units():
    """the product's units, and behind them the three scene libraries' own, the three lookup libraries', the tracked library's and
    the two delay libraries' (untagged build only)"""
    return _units() + ([] if TAG else [SCENE_UNIT, SCENE2_UNIT, SCENE3_UNIT] + LOOKUP_UNITS + LOOKUP3_UNITS + LOOKUP3P_UNITS + TRACKED_UNITS +
                       DELAY_UNITS + DELAY2_UNITS)


def _libs_exist() -> bool:
    return os.path.exists(LIB) and (bool(TAG) or all(os.path.exists(p) for p in (SCENE_LIB, SCENE2_LIB, SCENE3_LIB, LOOKUP_LIB,
                                                                               LOOKUP3_LIB, LOOKUP3P_LIB, TRACKED_LIB, DELAY_LIB,
                                                                               DELAY2_LIB)))


def _current_hashes() -> dict:
    return {src: _unit_hash(src, extra) for src, extra in _all_units()}


def _read_stamp() -> dict:
    try:
        with open(STAMP) as f:
            return json.load(f)
    except Exception:
        return {}


def is_current() -> bool:
    """True when libohs_hip.so (and, untagged, libohs_scene.so, libohs_scene2.so, libohs_scene3.so, libohs_lookup.so,
    libohs_lookup3.so, libohs_lookup3p.so, libohs_tracked.so, libohs_delay.so and libohs_delay2.so) exists and was built from exactly the sources in the tree."""
    return _libs_exist() and _read_stamp() == _current_hashes()


def build(force: bool = False, verbose: bool = False) -> str:
    units = _all_units()
    missing = [s for s, _ in units if not os.path.exists(os.path.join(CSRC, s))]
    if missing:
        raise RuntimeError(f"source files missing under {CSRC}: {missing}")
    want = _current_hashes()
    have = _read_stamp()
    if not force and _libs_exist() and have == want:
        return LIB
    os.makedirs(OBJ, exist_ok=True)
    hipcc = _hipcc()
    objs = []
    for src, extra in units:
        obj = os.path.join(OBJ, os.path.splitext(src)[0].replace("/", "_") + ".o")
        objs.append(obj)
        if force or not os.path.exists(obj) or _read_obj_hash(obj) != want[src]:
            cmd = [hipcc, *COMMON, *extra, *EXTRA_DEFS, "-Rpass-analysis=kernel-resource-usage", "-fno-caret-diagnostics", "-c",
                   os.path.join(CSRC, src), "-o", obj]
            if verbose:
                print(" ".join(cmd))
            r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
            remarks = [l for l in r.stderr.splitlines() if "-Rpass-analysis=kernel-resource-usage" in l]
            rest = [l for l in r.stderr.splitlines() if "-Rpass-analysis=kernel-resource-usage" not in l]
            if rest:
                sys.stderr.write("\n".join(rest) + "\n")
            if r.returncode != 0:
                raise subprocess.CalledProcessError(r.returncode, cmd)
            with open(obj + ".resources.json", "w") as f:
                json.dump(_parse_resource_remarks(remarks), f, indent=1, sort_keys=True)
            with open(obj + ".hash", "w") as f:
                f.write(want[src])
    # exported surface = the C ABI (csrc/exports.map); the C++ internals stay local
    n_product = len(_units())
    product_objs = objs[:n_product]
    links = [(LIB, product_objs, "exports.map")]
    if not TAG:     # the scene libraries: the same objects + api_scene.o / api_scene2.o / api_scene3.o, each its own version script
        links.append((SCENE_LIB, product_objs + [objs[n_product]], "scene_exports.map"))
        links.append((SCENE2_LIB, product_objs + [objs[n_product + 1]], "scene2_exports.map"))
        links.append((SCENE3_LIB, product_objs + [objs[n_product + 2]], "scene3_exports.map"))
        n_lookup = n_product + 3
        links.append((LOOKUP_LIB, objs[n_lookup:n_lookup + len(LOOKUP_UNITS)], "lookup_exports.map"))      # (its own objects only)
        n_lookup3 = n_lookup + len(LOOKUP_UNITS)
        links.append((LOOKUP3_LIB, objs[n_lookup3:n_lookup3 + len(LOOKUP3_UNITS)], "lookup3_exports.map"))  # (likewise)
        n_lookup3p = n_lookup3 + len(LOOKUP3_UNITS)
        links.append((LOOKUP3P_LIB, objs[n_lookup3p:n_lookup3p + len(LOOKUP3P_UNITS)], "lookup3p_exports.map"))   # (likewise)
        # the tracked library: the product's objects, the pruned lookup's kernels (not its C ABI) and its own two units
        n_tracked = n_lookup3p + len(LOOKUP3P_UNITS)
        n_delay = n_tracked + len(TRACKED_UNITS)
        links.append((TRACKED_LIB, product_objs + [objs[n_lookup3p]] + objs[n_tracked:n_delay], "tracked_exports.map"))
        links.append((DELAY_LIB, objs[n_delay:n_delay + len(DELAY_UNITS)], "delay_exports.map"))      # (its own objects only)
        n_delay2 = n_delay + len(DELAY_UNITS)
        links.append((DELAY2_LIB, objs[n_delay2:n_delay2 + len(DELAY2_UNITS)], "delay2_exports.map"))  # (likewise)
    for lib, lib_objs, vscript in links:
        cmd = [hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", lib, *lib_objs,
               "-Wl,--version-script=" + os.path.join(CSRC, vscript), "-lz", "-ldl", "-lpthread"]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
    res = {}
    for obj in objs:
        try:
            with open(obj + ".resources.json") as f:
                res.update(json.load(f))
        except Exception:       # noqa: BLE001 -- an object built before this file recorded them
            pass
    with open(RESOURCES, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    with open(STAMP, "w") as f:
        json.dump(want, f, indent=1)
    return LIB


def _parse_resource_remarks(lines: list[str]) -> dict:
    """{kernel (demangled base name, template arguments kept): {vgprs, agprs, sgprs, scratch_bytes_per_lane,
    lds_bytes, occupancy_waves_per_simd}} from hipcc's kernel-resource-usage remarks."""
    import re
    out, cur = {}, None
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "LDS Size [bytes/block]": "lds_bytes", "Occupancy [waves/SIMD]": "occupancy_waves_per_simd"}
    for l in lines:
        m = re.search(r"remark:\s+Function Name: (\S+)", l)
        if m:
            name = m.group(1)
            name = _kernel_base_name(name)
            cur = out.setdefault(name, {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", l)
        if m and cur is not None and m.group(1).strip() in keys:
            cur[keys[m.group(1).strip()]] = int(m.group(2))
    return out


def _kernel_base_name(mangled: str) -> str:
    """_ZN3ohs9k_conv_p1ENS_10ConvP1ArgsE -> k_conv_p1; _ZN3ohs9k_eq_passILi6EEEv... -> k_eq_pass<6> (Itanium
    nested-name <length><identifier> pairs; no demangler is needed for the kernels of this library)"""
    import re
    m = re.match(r"_ZN3ohs(\d+)", mangled)
    if not m:
        return mangled
    n = int(m.group(1))
    start = m.end()
    name = mangled[start:start + n]
    t = re.match(r"ILi(\d+)E", mangled[start + n:])
    return f"{name}<{t.group(1)}>" if t else name


def resources() -> dict:
    """the figures recorded by the last build (empty if the library was built before they were recorded)"""
    try:
        with open(RESOURCES) as f:
            return json.load(f)
    except Exception:           # noqa: BLE001
        return {}


def _read_obj_hash(obj: str) -> str:
    try:
        with open(obj + ".hash") as f:
            return f.read().strip()
    except Exception:
        return ""


def build_experiments(force: bool = False) -> str:
    """libohs_hip_exp.so beside the product library (a child process: this module's paths are fixed at import)"""
    env = dict(os.environ, OHS_BUILD_TAG="exp")
    env.pop("OHS_EXTRA_DEFS", None)
    cmd = [sys.executable, "-m", "open_headstage_amd.build"] + (["--force"] if force else [])
    subprocess.run(cmd, check=True, cwd=os.path.dirname(HERE), env=env, stdout=subprocess.DEVNULL)
    return os.path.join(HERE, "libohs_hip_exp.so")


def experiments_is_current() -> bool:
    r = subprocess.run([sys.executable, "-c", "import sys; from open_headstage_amd import build as b; sys.exit(0 if b.is_current() else 1)"],
                       cwd=os.path.dirname(HERE), env=dict(os.environ, OHS_BUILD_TAG="exp"))
    return r.returncode == 0


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
