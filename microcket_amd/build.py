"""Build every native artefact of the package in-tree (no JIT caches, nothing in site-packages).

    python -m microcket_amd.build            # library + executable
    python -m microcket_amd.build --all      # + oracle, reference build, test tools

libmkt_hip.so   hipcc --offload-arch=gfx950, hand-written HIP kernels + the C ABI (include/mkt.h)
bin/sam2pairs   the drop-in executable (same argv as the reference's bin/sam2pairs)
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libmkt_hip.so")
EXE = os.path.join(HERE, "bin", "sam2pairs")
ARCH = "gfx950"


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _run(cmd, **kw):
    print("+", " ".join(cmd), flush=True)
    subprocess.check_call(cmd, **kw)


def _headers():
    """Every header a native artefact may include: csrc/*.h (all of them, so that a new header can never be forgotten) + the ABI."""
    import glob
    return sorted(glob.glob(os.path.join(CSRC, "*.h"))) + sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: the HIP library cannot be built (there is no CPU build of this package)")


def _lib_sources():
    return [os.path.join(CSRC, f) for f in ("mkt_kernels.hip", "mkt_sort.hip", "mkt_rmdup.hip", "mkt_stitch.hip", "mkt_trim.hip", "mkt_bam.hip", "mkt_capi.cpp", "mkt_capi_ext.cpp", "mkt_capi_util.cpp", "mkt_matrix.hip", "mkt_layout.hip", "mkt_balance.hip", "mkt_expected.hip", "mkt_loops.hip", "mkt_eigs.hip", "mkt_insulation.hip", "mkt_pileup.hip", "mkt_saddle.hip", "mkt_scc.hip", "mkt_viewpoint.hip", "mkt_hic.hip", "mkt_deflate.hip", "mkt_paircmp.hip", "mkt_px2.hip", "mkt_inflate.hip", "mkt_bamtext.hip", "mkt_pairstat.hip")]


OBJ = os.path.join(HERE, "_build", "obj")
# sources whose host arithmetic is compared bit for bit with a numpy restatement: no fused multiply-add
EXACT_SOURCES = ("mkt_loops.hip", "mkt_insulation.hip", "mkt_pileup.hip", "mkt_saddle.hip", "mkt_scc.hip")
NO_CONTRACT = ("-ffp-contract=off",)


def _compile_objects(srcs, tag, flags):
    """One object per source (rebuilt only when it or a header is newer): a change in one file does not recompile the kernels."""
    os.makedirs(OBJ, exist_ok=True)
    hdrs = _headers()
    objs, procs = [], []
    for s in srcs:
        o = os.path.join(OBJ, tag + os.path.basename(s) + ".o")
        objs.append(o)
        if _newer(o, [s] + hdrs):
            own = NO_CONTRACT if os.path.basename(s) in EXACT_SOURCES else ()
            cmd = [hipcc(), "-c", "-fPIC", f"--offload-arch={ARCH}", "-O3", "-std=c++17", *flags, *own, "-Wno-unused-function", "-I" + CSRC, s, "-o", o]
            print("+", " ".join(cmd), flush=True)
            procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, pr in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    return objs


def build_lib(force=False):
    srcs = _lib_sources()
    deps = srcs + _headers()
    if force or _newer(LIB, deps):
        objs = _compile_objects(srcs, "", ("-Wall",))
        _run([hipcc(), "-shared", "-fPIC", f"--offload-arch={ARCH}", "-Wl,-rpath,/opt/rocm/lib", *objs, "-o", LIB])
    return LIB


def build_stamps_lib(name="libmkt_hip_stamps.so", defines=("-DMKT_STAMPS",)):
    """Diagnostic builds (phase stamps / phase ladder / tile-geometry experiments); never loaded by default."""
    out = os.path.join(HERE, name)
    srcs = _lib_sources()
    _run([hipcc(), "-shared", "-fPIC", f"--offload-arch={ARCH}", "-O3", "-std=c++17", *defines, "-Wno-unused-function",
          "-Wl,-rpath,/opt/rocm/lib", *srcs, "-o", out])
    return out


def build_variant(name, kernel_src=None, defines=()):
    """Experiment builds: another kernel source file and / or extra -D flags -> microcket_amd/<name> (select it with MKT_LIB)."""
    out = os.path.join(HERE, name)
    srcs = [kernel_src or os.path.join(CSRC, "mkt_kernels.hip")] + _lib_sources()[1:]
    _run([hipcc(), "-shared", "-fPIC", f"--offload-arch={ARCH}", "-O3", "-std=c++17", *defines, "-Wno-unused-function", "-I" + CSRC,
          "-Wl,-rpath,/opt/rocm/lib", *srcs, "-o", out])
    return out


def build_exe(force=False):
    src = os.path.join(CSRC, "sam2pairs_main.cpp")
    if force or _newer(EXE, [src, LIB] + _headers()):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", src, "-o", EXE, "-L" + HERE, "-lmkt_hip",
              "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    return EXE


PAIRSORT = os.path.join(HERE, "bin", "pairsort")


def build_pairsort(force=False):
    """bin/pairsort: the driver's sort / sort -m step on the GPU."""
    src = os.path.join(CSRC, "pairsort_main.cpp")
    if force or _newer(PAIRSORT, [src, LIB] + _headers()):
        os.makedirs(os.path.dirname(PAIRSORT), exist_ok=True)
        _run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", PAIRSORT, "-L" + HERE, "-lmkt_hip",
              "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    return PAIRSORT


KRMDUP = os.path.join(HERE, "bin", "krmdup")
KRMDUP_PIPE = os.path.join(HERE, "bin", "krmdup.pipe")


def build_krmdup(force=False):
    """bin/krmdup and bin/krmdup.pipe: drop-ins for the reference's FASTQ duplicate removal; one program,
    the interleaved-stdout form is chosen by its name."""
    src = os.path.join(CSRC, "krmdup_main.cpp")
    if force or _newer(KRMDUP, [src, LIB] + _headers()):
        os.makedirs(os.path.dirname(KRMDUP), exist_ok=True)
        _run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", KRMDUP, "-L" + HERE, "-lmkt_hip",
              "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    if force or _newer(KRMDUP_PIPE, [KRMDUP]):
        shutil.copy2(KRMDUP, KRMDUP_PIPE)
    return KRMDUP


STITCH = os.path.join(HERE, "bin", "stitch")


def build_stitch(force=False):
    """bin/stitch: the driver's `flash ... -To -c - | perl deal.flash.pl - PREFIX` step on the GPU (read stitching)."""
    src = os.path.join(CSRC, "stitch_main.cpp")
    if force or _newer(STITCH, [src, LIB] + _headers()):
        os.makedirs(os.path.dirname(STITCH), exist_ok=True)
        _run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", STITCH, "-L" + HERE, "-lmkt_hip",
              "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    return STITCH


KTRIM = os.path.join(HERE, "bin", "ktrim")


def build_ktrim(force=False):
    """bin/ktrim: the driver's `ktrim -k KIT -o PREFIX -1 R1 -2 R2 -c` step on the GPU (adapter and quality trimming);
    the reference's argv for the paired-end route, the same stdout and PREFIX.trim.log."""
    src = os.path.join(CSRC, "ktrim_main.cpp")
    if force or _newer(KTRIM, [src, LIB] + _headers()):
        os.makedirs(os.path.dirname(KTRIM), exist_ok=True)
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", src, "-o", KTRIM, "-L" + HERE, "-lmkt_hip",
              "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    return KTRIM


SAM2BAM = os.path.join(HERE, "bin", "sam2bam")


def build_sam2bam(force=False):
    """bin/sam2bam: the driver's `samtools view -b | samtools sort; samtools index` tail on the GPU."""
    src = os.path.join(CSRC, "sam2bam_main.cpp")
    if force or _newer(SAM2BAM, [src, LIB] + _headers()):
        os.makedirs(os.path.dirname(SAM2BAM), exist_ok=True)
        _run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", SAM2BAM, "-L" + HERE, "-lmkt_hip",
              "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    return SAM2BAM


PAIRS2MATRIX = os.path.join(HERE, "bin", "pairs2matrix")


def build_pairs2matrix(force=False):
    """bin/pairs2matrix: .pairs -> binned contact matrices (COO text, bins, counts) at several resolutions on the GPU: the
    computation behind the driver's `juicer_tools pre` / `cooler cload` stage (microcket:520-554)."""
    src = os.path.join(CSRC, "pairs2matrix_main.cpp")
    if force or _newer(PAIRS2MATRIX, [src, LIB] + _headers()):
        os.makedirs(os.path.dirname(PAIRS2MATRIX), exist_ok=True)
        _run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", PAIRS2MATRIX, "-L" + HERE, "-lmkt_hip",
              "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    return PAIRS2MATRIX


PAIRSCMP = os.path.join(HERE, "bin", "pairscmp")


def build_pairscmp(force=False):
    """bin/pairscmp: the reference's benchmarking/check.consistency.pl on the GPU (pair-level concordance of two .pairs files,
    DESIGN.md 6e); same argv, same stdout."""
    src = os.path.join(CSRC, "pairscmp_main.cpp")
    if force or _newer(PAIRSCMP, [src, LIB] + _headers()):
        os.makedirs(os.path.dirname(PAIRSCMP), exist_ok=True)
        _run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", PAIRSCMP, "-L" + HERE, "-lmkt_hip",
              "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    return PAIRSCMP


PAIRSBGZ = os.path.join(HERE, "bin", "pairsbgz")


def build_pairsbgz(force=False):
    """bin/pairsbgz: the driver's `bgzip -c final.pairs > final.pairs.gz; pairix final.pairs.gz` on the GPU: writes
    the BGZF file and its .px2 index."""
    src = os.path.join(CSRC, "pairsbgz_main.cpp")
    if force or _newer(PAIRSBGZ, [src, LIB] + _headers()):
        os.makedirs(os.path.dirname(PAIRSBGZ), exist_ok=True)
        _run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", PAIRSBGZ, "-L" + HERE, "-lmkt_hip",
              "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    return PAIRSBGZ


PAIRSGUNZIP = os.path.join(HERE, "bin", "pairsgunzip")


def build_pairsgunzip(force=False):
    """bin/pairsgunzip: the `bgzip -d -c` of this project (the BGZF inflate of DESIGN.md 6g): how a .pairs.gz reaches pairscmp."""
    src = os.path.join(CSRC, "pairsgunzip_main.cpp")
    if force or _newer(PAIRSGUNZIP, [src, LIB] + _headers()):
        os.makedirs(os.path.dirname(PAIRSGUNZIP), exist_ok=True)
        _run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", PAIRSGUNZIP, "-L" + HERE, "-lmkt_hip",
              "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    return PAIRSGUNZIP


PAIRSQUERY = os.path.join(HERE, "bin", "pairsquery")


def build_pairsquery(force=False):
    """bin/pairsquery: `pairix file.pairs.gz REGION ...` on the GPU (region queries through the .px2): only the blocks
    the index points to are inflated."""
    src = os.path.join(CSRC, "pairsquery_main.cpp")
    if force or _newer(PAIRSQUERY, [src, LIB] + _headers()):
        os.makedirs(os.path.dirname(PAIRSQUERY), exist_ok=True)
        _run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", PAIRSQUERY, "-L" + HERE, "-lmkt_hip",
              "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    return PAIRSQUERY


BAM2SAM = os.path.join(HERE, "bin", "bam2sam")


def build_bam2sam(force=False):
    """bin/bam2sam: the driver's `samtools view x.bam | sam2pairs /dev/stdin` front on the GPU (BGZF inflate, then BAM records to SAM
    text: DESIGN.md 6i); same stdout as `samtools view [-h | -H]`."""
    src = os.path.join(CSRC, "bam2sam_main.cpp")
    if force or _newer(BAM2SAM, [src, LIB] + _headers()):
        os.makedirs(os.path.dirname(BAM2SAM), exist_ok=True)
        _run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", BAM2SAM, "-L" + HERE, "-lmkt_hip",
              "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    return BAM2SAM


PAIRSSTAT = os.path.join(HERE, "bin", "pairsstat")


def build_pairsstat(force=False):
    """bin/pairsstat: pair-level QC of final.pairs on the GPU (distance by orientation, P(s), chromosome pairs: DESIGN.md 6k); writes
    PREFIX.pairs.stat and PREFIX.scaling.tsv."""
    src = os.path.join(CSRC, "pairsstat_main.cpp")
    if force or _newer(PAIRSSTAT, [src, LIB] + _headers()):
        os.makedirs(os.path.dirname(PAIRSSTAT), exist_ok=True)
        _run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", PAIRSSTAT, "-L" + HERE, "-lmkt_hip",
              "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    return PAIRSSTAT


MAKESTAT = os.path.join(HERE, "bin", "makestat")


def build_makestat(force=False):
    """bin/makestat: native stand-in for the reference's bin/make.stat.pl; host-only, no GPU library."""
    src = os.path.join(CSRC, "makestat_main.cpp")
    if force or _newer(MAKESTAT, [src]):
        os.makedirs(os.path.dirname(MAKESTAT), exist_ok=True)
        _run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", MAKESTAT])
    return MAKESTAT


def build_oracle():
    """Test infrastructure: CPU restatement (+ the reference itself when /root/reference is present)."""
    _run(["make", "-s", "-C", os.path.join(ROOT, "oracle")])


def build_emit_parts():
    """tests/host/emit_parts: host driver of the lean kernel's piecewise .pairs emitter (fast_emit_part in mkt_fast.h), plain and
    with the address and undefined-behaviour sanitizers (a stand-alone program: nothing of it is loaded into python)."""
    out = os.path.join(ROOT, "tests", "host", "_build")
    os.makedirs(out, exist_ok=True)
    src = os.path.join(ROOT, "tests", "host", "emit_parts.cpp")
    made = []
    for name, extra in (("emit_parts", ()), ("emit_parts_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))):
        exe = os.path.join(out, name)
        if os.path.exists(src) and _newer(exe, [src] + _headers()):
            _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *extra, "-o", exe, src])
        made.append(exe)
    return made


def build_parse_chain():
    """tests/host/parse_chain: host driver of what the lean kernel's heads phase leaves for its parser (fast_head_line) and of the
    parser's QNAME compare (lean_eq in mkt_fast.h), plain and with the address and undefined-behaviour sanitizers (a stand-alone
    program: nothing of it is loaded into python)."""
    out = os.path.join(ROOT, "tests", "host", "_build")
    os.makedirs(out, exist_ok=True)
    src = os.path.join(ROOT, "tests", "host", "parse_chain.cpp")
    made = []
    for name, extra in (("parse_chain", ()), ("parse_chain_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))):
        exe = os.path.join(out, name)
        if os.path.exists(src) and _newer(exe, [src] + _headers()):
            _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *extra, "-o", exe, src])
        made.append(exe)
    return made


def build_test_tools():
    out = os.path.join(ROOT, "tests", "host", "_build")
    os.makedirs(out, exist_ok=True)
    emul = os.path.join(out, "libmkt_emul.so")
    src = os.path.join(ROOT, "tests", "host", "tile_emul.cpp")
    if _newer(emul, [src] + _headers()):
        _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", emul, src])
    # host driver of the deflate code construction (mkt_deflate_codes.h); a tree that carries an older tests/ has no such source
    dzc = os.path.join(out, "deflate_codes")
    dsrc = os.path.join(ROOT, "tests", "host", "deflate_codes.cpp")
    if os.path.exists(dsrc) and _newer(dzc, [dsrc, os.path.join(CSRC, "mkt_deflate_codes.h")]):
        _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-o", dzc, dsrc])
    # host driver of read stitching's threshold table (mkt_stitch.h); a tree that carries an older tests/ has no such source
    sth = os.path.join(out, "stitch_thresholds")
    tsrc = os.path.join(ROOT, "tests", "host", "stitch_thresholds.cpp")
    if os.path.exists(tsrc) and _newer(sth, [tsrc, os.path.join(CSRC, "mkt_stitch.h"), os.path.join(ROOT, "include", "mkt.h")]):
        _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-o", sth, tsrc])
    # device check of the owning buffer types (mkt_devbuf.h): HIP runtime only; a tree that carries an older tests/ has no such source
    dbc = os.path.join(out, "devbuf_check")
    bsrc = os.path.join(ROOT, "tests", "host", "devbuf_check.cpp")
    if os.path.exists(bsrc) and _newer(dbc, [bsrc, os.path.join(CSRC, "mkt_devbuf.h")]):
        _run([hipcc(), f"--offload-arch={ARCH}", "-O1", "-g", "-std=c++17", "-Wall", "-Wl,-rpath,/opt/rocm/lib", "-o", dbc, bsrc])
    # host driver of the viewpoint profiles' host half (mkt_viewpoint.h), plain and with the address and undefined-behaviour sanitizers
    # (a stand-alone program: nothing of it is loaded into python); a tree that carries an older tests/ has no such source
    vsrc = os.path.join(ROOT, "tests", "host", "viewpoint_host.cpp")
    for name, extra in (("viewpoint_host", ()), ("viewpoint_host_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))):
        vph = os.path.join(out, name)
        if os.path.exists(vsrc) and _newer(vph, [vsrc, os.path.join(CSRC, "mkt_viewpoint.h"), os.path.join(ROOT, "include", "mkt.h")]):
            _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *extra, "-o", vph, vsrc])
    # host driver of the chunked text writer (mkt_chunked_file.h), plain and sanitized like the one above
    csrc = os.path.join(ROOT, "tests", "host", "chunked_file.cpp")
    for name, extra in (("chunked_file", ()), ("chunked_file_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))):
        chf = os.path.join(out, name)
        if os.path.exists(csrc) and _newer(chf, [csrc, os.path.join(CSRC, "mkt_chunked_file.h")]):
            _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *extra, "-o", chf, csrc])
    # host driver of the pair comparison's host half (mkt_paircmp.h: the report, the grouping by id string), plain and sanitized
    # like the ones above; a tree that carries an older tests/ has no such source
    psrc = os.path.join(ROOT, "tests", "host", "paircmp_host.cpp")
    for name, extra in (("paircmp_host", ()), ("paircmp_host_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))):
        pch = os.path.join(out, name)
        if os.path.exists(psrc) and _newer(pch, [psrc, os.path.join(CSRC, "mkt_paircmp.h"), os.path.join(ROOT, "include", "mkt.h")]):
            _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *extra, "-o", pch, psrc])
    # host driver of the pairs.gz index's host half (mkt_px2.h: the header, the reappearing-pair check), plain and sanitized like the
    # ones above; a tree that carries an older tests/ has no such source
    xsrc = os.path.join(ROOT, "tests", "host", "px2_host.cpp")
    for name, extra in (("px2_host", ()), ("px2_host_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))):
        pxh = os.path.join(out, name)
        if os.path.exists(xsrc) and _newer(pxh, [xsrc, os.path.join(CSRC, "mkt_px2.h")]):
            _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *extra, "-o", pxh, xsrc])
    # host driver of the BGZF reader's shared half (mkt_inflate.h: the block table, the header parse, the table build, the token
    # decode), plain and sanitized like the ones above; a tree that carries an older tests/ has no such source
    isrc = os.path.join(ROOT, "tests", "host", "inflate_host.cpp")
    for name, extra in (("inflate_host", ()), ("inflate_host_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))):
        ifh = os.path.join(out, name)
        if os.path.exists(isrc) and _newer(ifh, [isrc, os.path.join(CSRC, "mkt_inflate.h")]):
            _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *extra, "-o", ifh, isrc])
    # host driver of the region queries' host and shared half (mkt_px2query.h: the region grammar, the index kept, the block plan,
    # the line filter of the kernel), plain and sanitized like the ones above; a tree that carries an older tests/ has no such source
    qsrc = os.path.join(ROOT, "tests", "host", "pairsquery_host.cpp")
    for name, extra in (("pairsquery_host", ()), ("pairsquery_host_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))):
        pqh = os.path.join(out, name)
        if os.path.exists(qsrc) and _newer(pqh, [qsrc, os.path.join(CSRC, "mkt_px2query.h"), os.path.join(CSRC, "mkt_inflate.h")]):
            _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *extra, "-o", pqh, qsrc])
    # host driver of the BAM-to-SAM decoder's shared half (mkt_bamtext.h: the header walk, the record index with its resolve step, the
    # validation, length and emit routines of a record), plain and sanitized like the ones above; a tree that carries an older tests/
    # has no such source
    bsrc2 = os.path.join(ROOT, "tests", "host", "bamtext_host.cpp")
    for name, extra in (("bamtext_host", ()), ("bamtext_host_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))):
        bth = os.path.join(out, name)
        if os.path.exists(bsrc2) and _newer(bth, [bsrc2, os.path.join(CSRC, "mkt_bamtext.h")]):
            _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *extra, "-o", bth, bsrc2])
    # host driver of trimming's host half (mkt_trim.h: the argument check, the adapter table, the limit table, the record check, the
    # tail rule), plain and sanitized like the ones above; a tree that carries an older tests/ has no such source
    trsrc = os.path.join(ROOT, "tests", "host", "trim_host.cpp")
    for name, extra in (("trim_host", ()), ("trim_host_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))):
        trh = os.path.join(out, name)
        if os.path.exists(trsrc) and _newer(trh, [trsrc, os.path.join(CSRC, "mkt_trim.h"), os.path.join(ROOT, "include", "mkt.h")]):
            _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *extra, "-o", trh, trsrc])
    # host driver of the pair statistics' host and shared half (mkt_pairstat.h: the parse and the classes of a line, the areas, the
    # convergence rule, the two texts), plain and sanitized like the ones above; a tree that carries an older tests/ has no such source
    sssrc = os.path.join(ROOT, "tests", "host", "pairstat_host.cpp")
    for name, extra in (("pairstat_host", ()), ("pairstat_host_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))):
        psh = os.path.join(out, name)
        if os.path.exists(sssrc) and _newer(psh, [sssrc, os.path.join(CSRC, "mkt_pairstat.h"), os.path.join(CSRC, "mkt_chromtab.h"), os.path.join(CSRC, "mkt_core.h"), os.path.join(ROOT, "include", "mkt.h")]):
            _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *extra, "-o", psh, sssrc])
    build_emit_parts()
    build_parse_chain()
    tout = os.path.join(ROOT, "tools", "_build")
    os.makedirs(tout, exist_ok=True)
    synth = os.path.join(tout, "synth_sam")
    ssrc = os.path.join(ROOT, "tools", "synth_sam.cpp")
    if _newer(synth, [ssrc, os.path.join(CSRC, "mkt_synth.h")]):
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-o", synth, ssrc])


def build_all(force=False, extras=True):
    build_lib(force)
    build_exe(force)
    build_pairsort(force)
    build_krmdup(force)
    build_stitch(force)
    build_ktrim(force)
    build_sam2bam(force)
    build_pairs2matrix(force)
    build_pairscmp(force)
    build_pairsbgz(force)
    build_pairsgunzip(force)
    build_pairsquery(force)
    build_bam2sam(force)
    build_pairsstat(force)
    build_makestat(force)
    if extras:
        build_oracle()
        build_test_tools()


if __name__ == "__main__":
    build_all(force="--force" in sys.argv, extras="--all" in sys.argv or True)
