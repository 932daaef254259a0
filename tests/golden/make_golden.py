#!/usr/bin/env python3
"""Regenerate tests/golden/ref_components_{fast,ieee}.json.gz (and their textures / lights / spot_ies / cameras / integrator siblings, and
faure_tables.json.gz).

Runs ONLY in the build container (needs /root/reference).  It builds the component-level
reference harness (oracle/Makefile target `ref`: the reference's own sources compiled where they
lie, our driver oracle/ref_harness/ref_components.cc) in two flavours —

  fast : -O3 -ffast-math -DFAST_MATH -DFAST_TRIG   (the reference's release flags, CMakeLists.txt:241)
  ieee : -O2 -ffp-contract=off -DFAST_MATH -DFAST_TRIG

— runs both and stores their stdout (inputs + outputs as IEEE-754 bit patterns) as fixtures.
The fixtures are data; no reference source text is stored.  `faure` stores the reference's 50 Faure digit
permutations (the numbers of src/common/faure_tables.cc, in the order of its faure__ table) as a JSON list of lists.
"""
import gzip
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    if not os.path.isdir("/root/reference"):
        sys.exit("reference tree not present; fixtures can only be regenerated in the build container")
    which = sys.argv[1:] or ["components", "textures", "lights", "spot_ies", "cameras", "integrator", "integrator_lights", "faure"]
    if "faure" in which:
        which.remove("faure")
        faure()
    if which:
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True, timeout=900)
    ies_dir = tempfile.TemporaryDirectory()
    if "spot_ies" in which:     # the IES files the spot / IES harness reads: written here from tests/ies_fixture.py, named to the driver
        sys.path.insert(0, ROOT)
        from tests import ies_fixture
        for n in ies_fixture.SPECS:
            ies_fixture.write(ies_dir.name, n)
    for name in which:          # textures: image textures + shader nodes, oracle/ref_harness/ref_textures.cc
        for variant in ("fast", "ieee"):
            # integrator_lights: the integrator harness's second document (`ref_integrator lights`: the directional, sun and sphere light cases)
            exe, *args = (f"ref_{name}_{variant}",) if name != "integrator_lights" else (f"ref_integrator_{variant}", "lights")
            if name == "spot_ies":
                args = [ies_dir.name]
            out = subprocess.run([os.path.join(ROOT, "oracle", "_ref", exe), *args], check=True, capture_output=True, timeout=120).stdout
            out = out[out.index(b"{\n"):]          # the reference's handlers log to stdout before the document starts
            path = os.path.join(HERE, f"ref_{name}_{variant}.json.gz")
            with gzip.GzipFile(path, "wb", mtime=0) as f:
                f.write(out)
            print(path, len(out), "bytes raw")


def faure():
    # the reference tree the oracle Makefile's `ref` target compiles the other fixtures' harnesses from (its REF)
    ref = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "--eval", "print-ref: ; @echo $(REF)", "print-ref"],
                         check=True, capture_output=True, text=True).stdout.strip()
    txt = open(os.path.join(ref, "src", "common", "faure_tables.cc")).read()
    arrays = {int(m.group(1)): [int(v) for v in m.group(2).replace("\n", " ").split(",") if v.strip()]
              for m in re.finditer(r"int fp_(\d+)__\[\] = \{([^}]*)\}", txt)}
    order = re.search(r"faure__\[\] = \{([^}]*)\}", txt).group(1)
    names = [int(v) for v in re.findall(r"fp_(\d+)__", order)]
    path = os.path.join(HERE, "faure_tables.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps({"n_table_entries": len(names), "perms": [arrays[n] for n in names[:50]]}).encode())
    print(path, len(names), "table entries")


if __name__ == "__main__":
    main()
