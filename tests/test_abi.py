"""The C-ABI shared library loads without a GPU and exports every symbol include/derp_hip.h declares; the binding's
prototype table and struct mirrors say what the header says."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text():
    text = open(os.path.join(ROOT, "include", "derp_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declared_symbols():
    return sorted(set(re.findall(r"\b(derp_[a-z0-9_]+)\s*\(", header_text())))


# ---- the header, parsed: it is plain C, one `derp_name(args);` per declaration
STRUCT = re.compile(r"typedef\s+struct\s*\w*\s*\{([^}]*)\}\s*(derp_\w+)\s*;")
# header struct -> its ctypes mirror / its numpy dtype in facebook360_dep_amd.derp; a header struct in neither is listed
# in UNMIRRORED on purpose (none today)
MIRRORS = {"derp_camera_desc": "CameraDesc", "derp_options": "Options", "derp_render_params": "RenderParams",
           "derp_mesh_pass": "MeshPass", "derp_seq_options": "SeqOptions", "derp_seq_transfer": "SeqTransfer",
           "derp_isp_config": "IspConfig", "derp_sim_params": "SimParams"}
DTYPES = {"derp_sim_triangle": "SIM_TRIANGLE", "derp_sim_node": "SIM_NODE"}
UNMIRRORED = set()
SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
           "float": ctypes.c_float, "double": ctypes.c_double}
FIELDS = dict(SCALARS, **{"char": ctypes.c_char, "long long": ctypes.c_longlong})


def header_constants():
    """every enumerator of the header's (anonymous) enums -> its value"""
    out = {}
    for body in re.findall(r"\benum\s*\{([^}]*)\}", header_text()):
        value = -1
        for item in filter(None, (i.strip() for i in body.split(","))):
            name, _, given = (t.strip() for t in item.partition("="))
            value = int(given, 0) if given else value + 1
            out[name] = value
    return out


def header_structs():
    """{struct: [(field, scalar C type, (extents...))]} in declaration order"""
    constants = header_constants()
    out = {}
    for body, name in STRUCT.findall(header_text()):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            ctype, declarators = re.fullmatch(r"(long long|\w+)\s+(.*)", decl, flags=re.S).groups()
            for d in declarators.split(","):
                field, extents = re.fullmatch(r"\s*(\w+)((?:\[\w+\])*)\s*", d).groups()
                dims = tuple(int(e) if e.isdigit() else constants[e] for e in re.findall(r"\[(\w+)\]", extents))
                fields.append((field, ctype, dims))
        out[name] = fields
    return out


def header_prototypes():
    """{function: (return type, [parameter types])} as C spells them, `const` and the names dropped, no blanks at `*`"""
    text = STRUCT.sub("", header_text())
    text = re.sub(r"\benum\s*\{[^}]*\}\s*;|^\s*#.*$|extern\s+\"C\"\s*\{|typedef\s+struct\s+\w+\s+\w+\s*;", "", text, flags=re.M)

    def norm(t):
        return re.sub(r"\s*\*\s*", "*", " ".join(re.sub(r"\bconst\b", " ", t).split()))

    out = {}
    for decl in filter(None, (d.strip() for d in text.split(";"))):
        if decl == "}":  # the closing brace of extern "C"
            continue
        ret, name, params = re.fullmatch(r"(.*?)\b(derp_\w+)\s*\((.*)\)", decl, flags=re.S).groups()
        params = [] if params.strip() == "void" else [re.fullmatch(r"(.*?)\w+\s*", a, flags=re.S).group(1) for a in params.split(",")]
        assert name not in out, name
        out[name] = (norm(ret), [norm(a) for a in params])
    return out


def ctypes_of(c_type, derp):
    """The binding's rule for one C parameter or return type, restated: scalars by value keep their width; char* is
    c_char_p; a pointer to a struct with a ctypes mirror is POINTER(mirror); handles, T**, T* const* and every other
    data pointer are c_void_p."""
    if c_type == "void":
        return None
    if "*" not in c_type:
        return SCALARS[c_type]
    if c_type == "char*":
        return ctypes.c_char_p
    if c_type.count("*") == 1 and c_type[:-1] in MIRRORS:
        return ctypes.POINTER(getattr(derp, MIRRORS[c_type[:-1]]))
    return ctypes.c_void_p


def test_exports(built):
    from facebook360_dep_amd import derp

    lib = derp.lib()
    names = declared_symbols()
    assert len(names) >= 40
    for n in names:
        assert hasattr(lib, n), "libderp_hip.so does not export %s" % n
    assert sorted(derp.EXPORTS) == names, set(derp.EXPORTS) ^ set(names)


def test_prototypes_match_the_header(built):
    """restype and argtypes of every function on the loaded library are what the header declares: count, order, type."""
    from facebook360_dep_amd import derp

    lib = derp.lib()
    protos = header_prototypes()
    assert sorted(protos) == declared_symbols() and len(protos) >= 188
    for name, (ret, params) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is ctypes_of(ret, derp), (name, ret, fn.restype)
        assert fn.argtypes is not None, "%s has no argtypes" % name
        assert list(fn.argtypes) == [ctypes_of(p, derp) for p in params], (name, params, fn.argtypes)


def test_struct_mirrors_match_the_header(built):
    """Every struct of the header has a mirror with the same fields: names, order, scalar type and array extents."""
    import numpy as np

    from facebook360_dep_amd import derp

    structs = header_structs()
    assert set(structs) == set(MIRRORS) | set(DTYPES) | UNMIRRORED, set(structs) ^ (set(MIRRORS) | set(DTYPES) | UNMIRRORED)
    assert structs["derp_isp_config"][15] == ("rolloff_h", "float", (header_constants()["DERP_ISP_MAX_ROLLOFF"], 3))
    for name, mirror in MIRRORS.items():
        want = []
        for field, ctype, dims in structs[name]:
            t = FIELDS[ctype]
            for n in reversed(dims):
                t = t * n
            want.append((field, t))
        assert getattr(derp, mirror)._fields_ == want, name
    for name, mirror in DTYPES.items():
        dt = getattr(derp, mirror)
        base = {"float": np.dtype("<f4"), "int32_t": np.dtype("<i4")}
        assert list(dt.names) == [f for f, _, _ in structs[name]], name
        for field, ctype, dims in structs[name]:
            assert (dt[field].base, dt[field].shape) == (base[ctype], dims), (name, field)
        assert dt.itemsize == sum(4 * int(np.prod(dims, dtype=np.int64)) for _, _, dims in structs[name]), name


def test_argtypes_are_in_force(built):
    """A wrong kind of argument is refused at the boundary instead of reaching the C code (host-only function)."""
    import pytest

    from facebook360_dep_amd import derp

    width = ctypes.c_int()
    bounds = (ctypes.c_int * 4)(2, 10, 1, 5)
    with pytest.raises(ctypes.ArgumentError):
        derp.lib().derp_sweep_crop_size("8", bounds, ctypes.byref(width))
    with pytest.raises(ctypes.ArgumentError):
        derp.lib().derp_seq_owner(0, 9, 2, 0, 3.0)
    assert derp.lib().derp_sweep_crop_size(8, bounds, ctypes.byref(width)) == 0 and width.value > 0


def test_no_cpu_fallback(built):
    """Without a HIP device derp_create must fail loudly (no CPU compute path exists)."""
    import torch

    from facebook360_dep_amd import derp, synth

    if torch.cuda.is_available():
        return
    rig = synth.make_rig(4, 64)
    try:
        derp.Derp(rig["cameras"])
    except derp.DerpError as e:
        assert "no HIP device" in str(e) or "gfx950" in str(e)
    else:
        raise AssertionError("derp_create succeeded without a GPU")


def test_every_create_refuses_a_missing_device(built):
    """derp_create, derp_isp_create and derp_sim_create share one device check: without a HIP device each fails, hands
    back no handle and leaves "no HIP device" (and which path has no CPU fallback) in derp_last_error(NULL)."""
    import ctypes as C

    import torch

    from facebook360_dep_amd import derp, synth

    if torch.cuda.is_available():
        return
    lib = derp.lib()
    cams = (derp.CameraDesc * 2)(*[derp.camera_desc(c) for c in synth.make_rig(2, 64)["cameras"]])
    cfg = derp.isp_config({"width": 8, "height": 6})
    creates = (("the depth path", lambda h: lib.derp_create(C.byref(h), 0, cams, 2, cams, 2)),
               ("the ISP", lambda h: lib.derp_isp_create(C.byref(h), 0, C.byref(cfg), 0, 1, 1)),
               ("the simulator's tracer", lambda h: lib.derp_sim_create(C.byref(h), 0)))
    for path, create in creates:
        h = C.c_void_p()
        assert create(h) != 0 and not h.value, path
        message = lib.derp_last_error(None).decode()
        assert "no HIP device" in message and path in message and "no CPU fallback" in message, message


def test_product_does_not_touch_oracle():
    """The product package and the CLI sources never import / link the oracle."""
    pkg = os.path.join(ROOT, "facebook360_dep_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp", "Makefile")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle_lib" not in text and "derp_oracle" not in text and "libderp_oracle" not in text, f


def test_restated_libstdcxx_algorithms(built):
    """gcc_algos.h (what the device code runs) vs this image's libstdc++ through the oracle library."""
    import numpy as np

    from facebook360_dep_amd import derp
    from oracle import oracle_lib as O

    rng = np.random.default_rng(1)
    for t in range(4000):
        n = int(rng.integers(1, 33))
        if t % 3 == 0:
            p = rng.integers(0, 5, size=(n, 2)).astype(np.float32)  # many ties
        elif t % 3 == 1:
            p = np.sort(rng.random((n, 2)).astype(np.float32), axis=0)  # sorted input
        else:
            p = rng.random((n, 2)).astype(np.float32)
        nth = max(1, n - 2)
        assert np.array_equal(O.nth_element_pairs(p, nth), derp.host_nth_element_pairs(p, nth)), (n, p)
    for seed in (0, 1, 7, 12345, 2147483647, 2147483646):
        ref = O.minstd_uniform(seed, 64, 0.25, 1.75)
        got = np.array([derp.host_minstd_uniform(seed, i, 0.25, 1.75) for i in range(64)], dtype=np.float32)
        assert np.array_equal(ref, got), seed
    # jump-ahead far into the stream
    ref = O.minstd_uniform(99, 100001, 0.0, 1.0)
    assert ref[100000] == np.float32(derp.host_minstd_uniform(99, 100000, 0.0, 1.0))


def test_block_bias_rounding_identity():
    """k_random_proposals sums the 3x3 colour-bias boxes from the 4x4 texel block in fp32 and rounds with
    trunc((s + 4) * fl(1/9)) (derp_kernels.h, ssd_arith<RANDOM = true>); k_reproject_bias, like cv::blur on CV_16UC3
    (DerpUtil.cpp:208-210), rounds the integer sum with (s + 4) / 9. The two agree for EVERY possible sum of nine
    16-bit texels, and every such sum (+ 4) is exact in fp32."""
    import numpy as np

    s = np.arange(0, 9 * 65535 + 1, dtype=np.int64)
    f = s.astype(np.float32)
    assert np.array_equal(f.astype(np.int64), s) and np.array_equal((f + np.float32(4)).astype(np.int64), s + 4)
    q = np.trunc((f + np.float32(4)) * np.float32(1.0 / 9.0))
    assert q.dtype == np.float32 and np.array_equal(q.astype(np.int64), (s + 4) // 9)
