#!/bin/bash
# HBM traffic counters of the lz4 kernels at full size (separate --pmc passes, MI355X_MICROARCH.md HBM section)
out=$1
root=$(cd "$(dirname "$0")/.." && pwd)	# the repository: bench.py runs from there, $out is relative to it
cd /tmp && export TMPDIR=/tmp && cd "$root"
# (each pass under its own time limit; nothing more is started behind one that failed)
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $out/fetch -- python bench.py --steps 2 --warmup 1 --no-cpu-baseline > $out.fetch.log 2>&1 || exit 1
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $out/write -- python bench.py --steps 2 --warmup 1 --no-cpu-baseline > $out.write.log 2>&1 || exit 1
python - <<PY
import csv,glob,collections,json
res=collections.defaultdict(dict)
for p in ("fetch","write"):
    for f in glob.glob("$out/%s/*/*counter_collection.csv"%p):
        acc=collections.defaultdict(float); cnt=collections.Counter()
        for r in csv.DictReader(open(f)):
            k=r["Kernel_Name"].split("(")[0].replace("void ","")[:40]
            acc[k]+=float(r["Counter_Value"]); cnt[k]+=1
        for k in acc:
            if "lz4" in k or "scan" in k: res[k][p+"_kb_per_launch"]=acc[k]/cnt[k]; res[k]["launches"]=cnt[k]
import hashlib
import os
lib=os.environ.get("LA_GPU_LIB") or "libarchive_amd/csrc/libla_gpu.so"
res["library_sha16"]=hashlib.sha256(open(lib,"rb").read()).hexdigest()[:16]	# the build the counters belong to (bench.py compares)
k=[x for x in res if "lz4_expand_fast_kernel" in x and "false" in x]
if k:
    r=res[k[0]]
    # FETCH_SIZE counts half the bytes of wide coalesced reads on gfx950 (MI355X_MICROARCH.md, HBM): doubled; units KiB.
    # The window kernel's launches of a step are three contiguous slices and the groups of the split last slice
    # (la_lz4_slices.h), of unequal size, under one truncated name here: the figure is the kernel's bytes per STEP divided
    # by four, a quarter of the step like bench.py's algorithmic_bytes and launch_ms (launches_per_step: 4), so that it
    # stays comparable with the rounds that had four equal launches.  A step has one lz4_deps_kernel launch.
    steps=res.get("lz4_deps_kernel",{}).get("launches") or r.get("launches")/4
    per_launch=(2*r.get("fetch_kb_per_launch",0)+r.get("write_kb_per_launch",0))*1024
    res["lz4_expand_fast_kernel"]={"hbm_bytes_per_launch": per_launch*r.get("launches")/steps/4, "launches": r.get("launches"), "steps": steps,
        "note": "bytes per step / 4: the step's window launches are unequal since the last slice is split"}
print(json.dumps(res, indent=1))
PY
