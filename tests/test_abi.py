"""
The C ABI seen by three consumers must be ONE layout ("ctypes structs and Julia structs are hand-mirrored from the
header; no compiled-C consumer pins sizeof/offsetof"):
  * tests/abi_layout.c, compiled with gcc against include/octofitter_hip.h, prints sizeof/offsetof of every struct and
    dlopens the library (CPU: every declared symbol resolves; GPU: one octo_eval call through plain C);
  * the ctypes mirror (octofitter.jl_amd/host/capi.py) must agree field by field;
  * the Julia mirror (octofitter.jl_amd/julia/OctofitterHIP.jl — Julia is not in the image, so its struct definitions are parsed
    as text and laid out by the C rules for Int32 / Int64 / Float64 / Ptr) must agree field by field, the shim must `ccall`
    every function the header declares with the right number of arguments, and every numeric constant it repeats must match.
"""
import ctypes as C
import json
import os
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "octofitter_hip.h"
JULIA = ROOT / "octofitter.jl_amd" / "julia" / "OctofitterHIP.jl"
JULIA_CAPI = ROOT / "octofitter.jl_amd" / "julia" / "OctofitterHIP_capi.jl"      # the thin layer: constants, structs, one ccall per symbol


def _julia_text():
    """The shim as Julia sees it: OctofitterHIP.jl with its include of the ccall layer expanded."""
    main = JULIA.read_text()
    inc = 'include("OctofitterHIP_capi.jl")'
    assert main.count(inc) == 1, "OctofitterHIP.jl includes the ccall layer exactly once"
    return main.replace(inc, JULIA_CAPI.read_text())


@pytest.fixture(scope="module")
def abi_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("abi") / "abi_layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", "-o", str(exe), str(ROOT / "tests" / "abi_layout.c"), "-ldl"], check=True)
    return exe


@pytest.fixture(scope="module")
def layout(abi_exe):
    return json.loads(subprocess.run([str(abi_exe), "layout"], check=True, capture_output=True, text=True).stdout)


def _header_functions():
    """name -> number of parameters of every function the header declares."""
    txt = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int32_t|int64_t|const char\*)\s+(octo_\w+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len([a for a in args.split(",") if a.strip()])
    return out


def test_c_program_sees_every_symbol(pkg, abi_exe, layout):
    funcs = _header_functions()
    assert layout["n_symbols"] == len(funcs), "tests/abi_layout.c SYMBOLS and the header disagree"
    assert set(funcs) == set(pkg.capi.EXPORTED_SYMBOLS), set(funcs) ^ set(pkg.capi.EXPORTED_SYMBOLS)
    r = subprocess.run([str(abi_exe), "symbols", str(pkg.capi.LIB_PATH)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout)["symbols_ok"] == len(funcs)
    for name, (res, args) in pkg.capi._SIGS.items():      # the ctypes signatures have the header's arity
        assert len(args) == funcs[name], (name, len(args), funcs[name])


def test_ctypes_structs_match_the_header(pkg, layout):
    capi = pkg.capi
    pairs = {"octo_consts": capi.OctoConsts, "octo_obs_desc": capi.OctoObsDesc, "octo_planet_desc": capi.OctoPlanetDesc,
             "octo_prior": capi.OctoPrior, "octo_source": capi.OctoSource}
    for cname, cls in pairs.items():
        ref = layout[cname]
        assert C.sizeof(cls) == ref["size"], cname
        assert [f[0] for f in cls._fields_] == [f[0] for f in ref["fields"]], cname
        for (fname, _), (rname, off, size) in zip(cls._fields_, ref["fields"]):
            d = getattr(cls, fname)
            assert (d.offset, d.size) == (off, size), (cname, fname)
    assert (capi.N_EL, capi.N_NUIS) == (layout["OCTO_N_EL"], layout["OCTO_N_NUIS"])


_JL_SIZES = {"Int32": 4, "Int64": 8, "Float64": 8, "UInt64": 8}


def _julia_structs():
    txt = _julia_text()
    out = {}
    for m in re.finditer(r"^struct (Octo\w+)[ \t]*(?:#[^\n]*)?\n(.*?)^end", txt, flags=re.S | re.M):
        fields = []
        for line in m.group(2).splitlines():
            line = line.split("#")[0].strip()
            for part in filter(None, (p.strip() for p in line.split(";"))):
                name, typ = part.split("::")
                fields.append((name.strip(), typ.strip()))
        out[m.group(1)] = fields
    return out


def test_julia_structs_match_the_header(layout):
    structs = _julia_structs()
    pairs = {"octo_consts": "OctoConsts", "octo_obs_desc": "OctoObsDesc", "octo_planet_desc": "OctoPlanetDesc", "octo_prior": "OctoPrior",
             "octo_source": "OctoSource"}
    for cname, jname in pairs.items():
        assert jname in structs, f"{jname} missing from OctofitterHIP.jl"
        ref = layout[cname]
        off = 0
        align_max = 1
        assert [f[0] for f in structs[jname]] == [f[0] for f in ref["fields"]], (jname, "field names / order")
        for (fname, typ), (_, roff, rsize) in zip(structs[jname], ref["fields"]):
            size = 8 if typ.startswith("Ptr{") else _JL_SIZES[typ]
            off = (off + size - 1) // size * size          # natural alignment, as Julia lays out isbits structs (C-compatible)
            align_max = max(align_max, size)
            assert (off, size) == (roff, rsize), (jname, fname, typ)
            off += size
        assert (off + align_max - 1) // align_max * align_max == ref["size"], jname


def test_julia_shim_binds_every_symbol_with_the_right_arity():
    funcs = _header_functions()
    txt = _julia_text()
    seen = {}
    for m in re.finditer(r"ccall\(\(:(octo_\w+), LIB\),\s*\w+,\s*\(", txt):
        # argument-type tuple: balanced parentheses after the return type
        i = m.end()
        depth, j = 1, i
        while depth:
            depth += {"(": 1, ")": -1}.get(txt[j], 0)
            j += 1
        tup = txt[i:j - 1]
        depth, n, cur = 0, 0, ""
        for ch in tup:
            if ch in "({":
                depth += 1
            elif ch in ")}":
                depth -= 1
            if ch == "," and depth == 0:
                n += bool(cur.strip()); cur = ""
            else:
                cur += ch
        n += bool(cur.strip())
        seen.setdefault(m.group(1), set()).add(n)
    missing = set(funcs) - set(seen)
    assert not missing, f"OctofitterHIP.jl has no ccall for {sorted(missing)}"
    for name, counts in seen.items():
        assert name in funcs, f"OctofitterHIP.jl calls {name}, which the header does not declare"
        assert counts == {funcs[name]}, (name, counts, funcs[name])


def test_julia_constants_match_the_header():
    hdr = HEADER.read_text()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(OCTO_\w+)\s+(-?\d+)\b", hdr)}
    txt = _julia_text()
    groups = {
        "ASTROM_RADEC, ASTROM_SEPPA, RV_ABS, RV_ABS_MARG, RV_REL": ["OCTO_ASTROM_RADEC", "OCTO_ASTROM_SEPPA", "OCTO_RV_ABS", "OCTO_RV_ABS_MARG", "OCTO_RV_REL"],
        "ONEIL_RADEC, ONEIL_SEPPA, HGCA": ["OCTO_ONEIL_RADEC", "OCTO_ONEIL_SEPPA", "OCTO_HGCA"],
        "ORBIT_VISUAL_KEP, ORBIT_RADVEL, ORBIT_THIELE_INNES, ORBIT_KEP": ["OCTO_ORBIT_VISUAL_KEP", "OCTO_ORBIT_RADVEL", "OCTO_ORBIT_THIELE_INNES", "OCTO_ORBIT_KEP"],
        "PRIOR_UNIFORM, PRIOR_LOGUNIFORM, PRIOR_NORMAL, PRIOR_TRUNCNORMAL, PRIOR_SINE": ["OCTO_PRIOR_UNIFORM", "OCTO_PRIOR_LOGUNIFORM", "OCTO_PRIOR_NORMAL",
                                                                                         "OCTO_PRIOR_TRUNCNORMAL", "OCTO_PRIOR_SINE"],
        "SRC_CONST, SRC_THETA, SRC_CIRCULAR, SRC_TPERI": ["OCTO_SRC_CONST", "OCTO_SRC_THETA", "OCTO_SRC_CIRCULAR", "OCTO_SRC_TPERI"],
        "SRC_FLAG_UNITLEN, SRC_FLAG_TI": ["OCTO_SRC_FLAG_UNITLEN", "OCTO_SRC_FLAG_TI"],
        "OCTO_OK, OCTO_EINVAL, OCTO_EHIP, OCTO_ENOMEM, OCTO_ENODEV, OCTO_ENOTSUP": ["OCTO_OK", "OCTO_EINVAL", "OCTO_EHIP", "OCTO_ENOMEM", "OCTO_ENODEV", "OCTO_ENOTSUP"],
    }
    for lhs, names in groups.items():
        m = re.search(r"const " + re.escape(lhs) + r"\s*=\s*(.+)", txt)
        assert m, lhs
        vals = [int(v) for v in re.findall(r"Int32\((-?\d+)\)", m.group(1))]
        assert vals == [defs[n] for n in names], (lhs, vals)
    assert re.search(r"const N_EL, N_NUIS = (\d+), (\d+)", txt).groups() == (str(defs["OCTO_N_EL"]), str(defs["OCTO_N_NUIS"]))


def test_julia_shim_names_exist_in_the_reference():
    """745+ lines of Julia that cannot run in the build image: every `Octofitter.<name>` the shim calls or extends and every
    field it reads from a reference struct (`obs.trend_function`, `obs.gaussian_process`, `obs.wrapped_like`, `model.arr2nt`, table
    columns, …) must be a name the reference defines. tools/julia_api_manifest.py extracts both sides; the committed manifest
    (tests/golden/julia_api_names.json: name -> defining file:line) is DATA that travels; when OCTOFITTER_REFERENCE_DIR names a checkout of
    the reference, the manifest itself is re-derived and every entry re-checked against the sources, so API drift on either side fails here."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("julia_api_manifest", ROOT / "tools" / "julia_api_manifest.py")
    jm = importlib.util.module_from_spec(spec); spec.loader.exec_module(jm)
    man = json.loads((ROOT / "tests" / "golden" / "julia_api_names.json").read_text())
    qualified, imported, own_fields, fields = jm.shim_names(_julia_text())
    assert {"ln_like", "likelihoodname", "_isprior", "likeobj_from_epoch_subset", "orbittype", "make_arr2nt", "make_prior_sampler"} <= qualified
    missing = sorted(n for n in qualified | imported if n not in man["names"])
    assert not missing, f"OctofitterHIP.jl uses Octofitter names the manifest does not know: {missing} (run tools/julia_api_manifest.py)"
    need = (fields - own_fields - jm.THETA_FIELDS - jm.OTHER_FIELDS - jm.EXTERNAL) | set(jm.REQUIRED_REFERENCE_FIELDS)
    missing = sorted(n for n in need if n not in man["fields"])
    assert not missing, f"OctofitterHIP.jl reads fields the manifest does not know: {missing} (run tools/julia_api_manifest.py)"
    for must in ("trend_function", "gaussian_process", "wrapped_like", "hgca", "dist_hip", "table", "priors", "derived"):
        assert must in man["fields"], must
    ref = os.environ.get("OCTOFITTER_REFERENCE_DIR")
    if not ref:
        return                                          # no reference checkout named: the manifest is the travelling record
    jm.REF = Path(ref)
    fresh, not_found = jm.build()
    assert not not_found, f"names the reference does not define: {not_found}"
    assert fresh["names"] == man["names"] and fresh["fields"] == man["fields"], "tests/golden/julia_api_names.json is stale: run tools/julia_api_manifest.py"
    for name, where in list(man["names"].items()) + list(man["fields"].items()):
        path, line = where.split(" ")[0].rsplit(":", 1)
        src = (jm.REF / path).read_text(errors="replace").splitlines()
        assert name in src[int(line) - 1], (name, where)


def test_julia_shim_classifies_the_trend_closure():
    """The boundary defect of VERDICT r2: `_table` took every RV observation without a GP, although `trend_function` is always a closure
    (rv-absolute.jl:69). Structural check of the fix: the RV branch goes through `_trend_basis`, an unclassifiable closure makes the
    observation ineligible (`return nothing`), the basis column is uploaded as `extra`, and the coefficient reaches the third nuisance row."""
    txt = _julia_text()
    rv = txt[txt.index("kind = T === :StarAbsoluteRVObs"):txt.index("_has_epochs(obs) =")]
    assert "_trend_basis(obs, θobs_draws)" in rv and "tb === nothing && return nothing" in rv and "gaussian_process" in rv
    assert rv.index("gaussian_process") < rv.index("_trend_basis")
    tb = txt[txt.index("function _trend_basis"):txt.index("function _table")]
    assert "obs.trend_function" in tb and "all(iszero, v)" in tb and "return nothing" in tb
    assert "getproperty(θobs, trendcoef)" in txt and "_eligible(obs, ip, θs)" in txt
    assert "_table(obs, 1) !== nothing" not in txt      # the old, θ-blind eligibility test is gone


@pytest.mark.gpu
def test_plain_c_consumer_evaluates(pkg, abi_exe):
    r = subprocess.run([str(abi_exe), "eval", str(pkg.capi.LIB_PATH)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    out = json.loads(r.stdout)
    assert out["ok"] == 1 and out["ll1_is_minus_inf"] == 1


def test_julia_ccall_layer_is_thin_and_self_contained():
    """SURVEY.md §7 asks for a thin, pure-`ccall` shim: the layer a maintainer needs to reach the C ABI from Julia is ONE file of about 200 lines
    that names nothing of Octofitter (no `Octofitter.`, no `using`), holds every `ccall` of the binding, and nothing but constants, structs
    and call wrappers; everything that touches the reference's types lives in OctofitterHIP.jl on top of it."""
    capi = JULIA_CAPI.read_text()
    code = [l for l in capi.splitlines() if l.strip() and not l.lstrip().startswith("#")]
    assert len(code) <= 200, len(code)
    assert "Octofitter." not in capi.replace("OctofitterHIP", "") and not re.search(r"^\s*using\s", capi, re.M)
    main = JULIA.read_text()
    assert "ccall(" not in main, "every ccall belongs to the thin layer"
    assert not re.search(r"^\s*(mutable\s+)?struct\s+Octo[A-Z]\w*", main, re.M), "the header's structs are mirrored in the thin layer"


def test_julia_shim_falls_back_instead_of_throwing():
    """the shim "falls back to the reference closure when any observation is ineligible" — VERDICT r4: `accelerate(system)` on a
    system of more planets than the kernels take, or on a host without a usable GPU, used to reach octo_dataset_create / octo_ctx_create -> check -> error(), leaking the
    context. Structural check (Julia is not in the image) of the three branches and of the failure paths' clean-up:
      * more planets than OCTO_MAX_PLANETS (the reference unrolls over any number, src/likelihoods/system.jl:116-118): decided on the host
        BEFORE anything is created;
      * no usable device / a refused dataset: the library's status arrives as a typed `OctoError` (not a bare `error`), `accelerate` and
        `HIPLogDensityModel` catch exactly that, log one `@info` and return the object they were given;
      * `_upload` destroys the context it created when the dataset is refused; a failed extra slot destroys its context too."""
    capi = JULIA_CAPI.read_text()
    main = JULIA.read_text()
    hdr = HEADER.read_text()
    n_max = int(re.search(r"#define\s+OCTO_MAX_PLANETS\s+(\d+)", hdr).group(1))
    assert re.search(rf"const OCTO_MAX_PLANETS = {n_max}\b", capi)
    # typed exception, thrown by every status check and by octo_ctx_create
    assert re.search(r"struct OctoError <: Exception\s+status::Int32", capi)
    assert "throw(OctoError(st, what" in capi and 'throw(OctoError(st, "octo_ctx_create"' in capi
    assert not re.search(r"(?<![A-Za-z_.])error\(", capi), "the ccall layer reports library failures as OctoError only"
    # the host-side planet-count rule
    m = re.search(r"function _not_on_device\(system\)(.*?)\nend\n", main, re.S)
    assert m and "length(system.planets)" in m.group(1) and "np > OCTO_MAX_PLANETS" in m.group(1)
    # _upload: context destroyed on the failure path
    up = re.search(r"function _upload\(.*?\n(.*?)\nend\n", main, re.S).group(1)
    assert re.search(r"ctx = octo_ctx_create\(device\)\s+try\b.*octo_dataset_create\(ctx.*catch\s+octo_ctx_destroy\(ctx\).*rethrow\(\)", up, re.S)
    # accelerate: the three branches, each returning `system`
    acc = re.search(r"function accelerate\(system::System;.*?\n(.*?)\n    n_in = ", main, re.S).group(1)
    assert re.search(r"why = _not_on_device\(system\)\s+if why !== nothing.*?@info.*?return system\s+end", acc, re.S)
    assert re.search(r"try\s+ctx, ds, entries, columns = _upload\(.*?catch e\s.*?is_fallback\(e\) \|\| rethrow\(\).*?@info.*?return system\s+end", acc, re.S)
    slots = re.search(r"for _ in 2:max\(1, n_contexts\)(.*?)\n    end\n", main, re.S).group(1)
    assert "octo_ctx_destroy(c)" in slots and "e isa OctoError || rethrow()" in slots and "break" in slots
    # the fallback answers ONLY "no device" / "a valid system that is not on the device path" / the shim's own NotOnHIPPath — bad input
    # (OCTO_EINVAL), OCTO_EHIP, OCTO_ENOMEM and plain ErrorExceptions (bugs) are rethrown
    capi_txt = JULIA_CAPI.read_text()
    assert re.search(r"is_fallback\(e\) = e isa NotOnHIPPath \|\| \(e isa OctoError && \(e.status == OCTO_ENODEV \|\| e.status == OCTO_ENOTSUP\)\)", capi_txt)
    assert "ErrorException" not in main.replace("# ", "")
    # HIPLogDensityModel: returns the reference's model
    h = re.search(r"function HIPLogDensityModel\(model;.*?\n(.*?)\nend\n", main, re.S).group(1)
    assert "_not_on_device(model.system)" in h and "is_fallback(e) || rethrow()" in h and "@info" in h and h.rstrip().endswith("return model")
    assert "fallback || return _hip_log_density_model(model; device)" in h


def test_julia_pigeons_driver_calls_what_is_bound_and_follows_the_shared_protocol():
    """the batched parallel-tempering driver of julia/OctofitterHIP.jl (octofit_pigeons_hip) cannot run here, so it is held
    statically: every octo_* call in its body is a wrapper the ccall layer defines, with that wrapper's positional arity; the reference function it
    reaches for exists (tests/golden/julia_api_names.json); and the protocol constants it shares with its executable twin host/tempering.py
    (TemperedSwap: the ladder, the walker layout r_local·n_chains + c, parity = scan % 2, the [n_chains][n_temps] label matrix) agree."""
    main = (ROOT / "octofitter.jl_amd" / "julia" / "OctofitterHIP.jl").read_text()
    capi_txt = JULIA_CAPI.read_text()
    body = re.search(r"function octofit_pigeons_hip\(.*?\n(.*?)\nend\n\nexport octofit_pigeons_hip", main, re.S).group(1)

    def arity(sig):      # top-level commas of an argument list, keyword part (after ';') dropped
        sig = sig.split(";")[0]
        depth, n, cur = 0, 0, ""
        for ch in sig:
            depth += ch in "([{"; depth -= ch in ")]}"
            if ch == "," and depth == 0:
                n += bool(cur.strip()); cur = ""
            else:
                cur += ch
        return n + bool(cur.strip())

    def call_args(text, start):
        depth, j = 1, start
        while depth:
            depth += {"(": 1, ")": -1}.get(text[j], 0); j += 1
        return text[start:j - 1]
    defs = {}
    for m in re.finditer(r"^(?:function )?(octo_\w+!?)\(", capi_txt, re.M):
        defs.setdefault(m.group(1), set()).add(arity(call_args(capi_txt, m.end())))
    calls = [(m.group(1), arity(call_args(body, m.end()))) for m in re.finditer(r"\b(octo_\w+!?)\(", body)]
    assert {c[0] for c in calls} >= {"octo_comm_unique_id", "octo_comm_create", "octo_model_logpost!", "octo_pt_step", "octo_comm_destroy"}, calls
    for name, n in calls:
        assert name in defs, f"octofit_pigeons_hip calls {name}, which OctofitterHIP_capi.jl does not define"
        assert n in defs[name] or any(n <= d for d in defs[name]), (name, n, defs[name])      # (trailing defaulted arguments may be omitted)
    man = json.loads((ROOT / "tests" / "golden" / "julia_api_names.json").read_text())
    assert "make_ln_prior_transformed" in man["names"], "the reference's prior density constructor the driver calls (src/logdensitymodel.jl:47)"
    twin = (ROOT / "octofitter.jl_amd" / "host" / "tempering.py").read_text()
    assert "range(1.0, 0.0; length=n_temps)) .^ 3" in body and "linspace(1.0, 0.0, self.n_temps, dtype=torch.float64) ** 3" in twin      # the same ladder
    assert "r * n_chains + c" in body and "r_local * n_chains + c" in twin                                                                # the same walker layout
    assert "scan % 2" in body and "int(step) % 2" in twin                                                                                 # the same parity rule
    assert "octo_pt_step(" in twin.replace("lib.octo_pt_step(", "octo_pt_step(")
