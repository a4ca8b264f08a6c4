"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every symbol that
include/ebfi_hip.h declares, the ctypes table derived from that header covers all of them with the
right types, and the product ops fail loudly (never fall back) when handed CPU tensors.  No compute calls: there is no GPU here."""
import ctypes
import os

import pytest
import torch

from ebfi_amd import _native as N


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.LIB_PATH


def test_header_symbols_all_bound():
    declared = N.declared_symbols()
    assert len(declared) >= 16
    assert set(declared) == set(N.SIGNATURES), (set(declared) ^ set(N.SIGNATURES))


def test_library_exports_every_declared_symbol(built_lib):
    h = ctypes.CDLL(built_lib)
    for name in N.declared_symbols():
        assert hasattr(h, name), name


def test_library_loads_and_reports_version(built_lib):
    lib = N.lib()
    # the binding, the header and the library agree on the ABI generation (14 since the two-part image writer of round 6)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ebfi_hip.h")).read()
    assert "#define EBFI_ABI_VERSION 14" in header
    assert lib.ebfi_abi_version() == 14 == N.ABI_VERSION
    assert lib.ebfi_events_workspace(16) == (2 * 16 + 1) * 8
    # workspace query is pure host arithmetic: 512 slabs max, here 2*ceil(16/64)=2 tiles -> 2 slabs
    need = lib.ebfi_dcn_backward_workspace(2, 2, 4, 4, 2, 3, 3, 1, 1, 1, 1, 1, 1, 1, 0)
    assert need == 2 * (2 * 2 * 9 + 2) * 4


def test_argument_errors_do_not_touch_the_gpu(built_lib):
    lib = N.lib()
    bad = N.i64x4((1, 1, 4, 4))
    rc = lib.ebfi_fac_forward(None, bad, bad, None, bad, bad, 3, None, bad, bad, 0, None)
    assert rc == -1 and b"null" in lib.ebfi_last_error()
    rc = lib.ebfi_dcn_forward(*([ctypes.c_void_p(8)] * 6), 1, 3, 4, 4, 2, 3, 3, 1, 1, 1, 1, 1, 1, 2, 0, None)
    assert rc == -1 and b"divisible" in lib.ebfi_last_error()
    rc = lib.ebfi_dcn_forward(*([ctypes.c_void_p(8)] * 6), 1, 2, 4, 4, 2, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, None)
    assert rc == -3    # a dtype code other than EBFI_F32 -> loud, not silent


def test_ops_refuse_cpu_tensors():
    from ebfi_amd.dcn import dcn_v2_conv
    from ebfi_amd.encodings import events_to_stack
    from ebfi_amd.fac import KernelConv2D
    from ebfi_amd.blur import Frame2Lap
    with pytest.raises(NotImplementedError):
        KernelConv2D(3)(torch.randn(1, 2, 4, 4), torch.randn(1, 18, 4, 4))
    with pytest.raises(NotImplementedError):
        dcn_v2_conv(torch.randn(1, 2, 4, 4), torch.zeros(1, 18, 4, 4), torch.ones(1, 9, 4, 4),
                    torch.randn(2, 2, 3, 3), torch.zeros(2), 1, 1, 1, 1)
    with pytest.raises(NotImplementedError):
        events_to_stack(torch.zeros(5), torch.zeros(5), torch.zeros(5), torch.zeros(5), 4, (4, 4))
    with pytest.raises(NotImplementedError):
        Frame2Lap(torch.rand(1, 3, 4, 4))


def test_missing_library_is_loud(monkeypatch, tmp_path):
    monkeypatch.setattr(N, "_lib", None)
    monkeypatch.setattr(N, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(N.EbfiNativeError):
        N.lib()


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ebfi-be_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".sh")):
                text = open(os.path.join(root, f)).read()
                assert "import oracle" not in text and "from oracle" not in text, os.path.join(root, f)
                assert "liboracle" not in text, os.path.join(root, f)


# ------------------------------------------------------------------ the binding is derived from the header
_c = ctypes
_vp, _i, _i64, _p64 = _c.c_void_p, _c.c_int, _c.c_int64, _c.POINTER(_c.c_int64)

SYNTHETIC = """
/* a comment that looks like code: int ebfi_in_block_comment(int a); */
// int ebfi_in_line_comment(int a);
#ifndef X_H
#define X_H
#ifdef __cplusplus
extern "C" {
#endif
#define EBFI_LIMIT 7
#define EBFI_MASK 0x10
typedef enum { EBFI_OK = 0, EBFI_ERR_A = -1, EBFI_ERR_B = -2 } ebfi_status;
enum { EBFI_FIRST, EBFI_SECOND, EBFI_TENTH = 10, EBFI_ELEVENTH };
int ebfi_spread(const void *input,   /* device */
                const int64_t shape[4],
                float slope,
                void *stream);
const char *ebfi_text(void);
void ebfi_nothing(void);
size_t ebfi_lists(int n, const void *const *ins, void *const *outs, const float *w, uint8_t *bytes, uint64_t seed, double t,
                  int64_t count);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_rules_on_a_synthetic_header():
    sig, params, const = N.parse_header(SYNTHETIC)
    assert sig == {
        "ebfi_spread": (_i, [_vp, _p64, _c.c_float, _vp]),                 # four lines, an array parameter
        "ebfi_text": (_c.c_char_p, []),                                   # (void)
        "ebfi_nothing": (None, []),
        "ebfi_lists": (_c.c_size_t, [_i, _vp, _vp, _vp, _vp, _c.c_uint64, _c.c_double, _i64]),    # const void *const *
    }
    assert params["ebfi_spread"] == ["const void *input", "const int64_t shape[4]", "float slope", "void *stream"]
    assert params["ebfi_text"] == []
    assert const == {"EBFI_LIMIT": 7, "EBFI_MASK": 16, "EBFI_OK": 0, "EBFI_ERR_A": -1, "EBFI_ERR_B": -2,
                     "EBFI_FIRST": 0, "EBFI_SECOND": 1, "EBFI_TENTH": 10, "EBFI_ELEVENTH": 11}


@pytest.mark.parametrize("proto, names", [
    ("int ebfi_bad(const void *a, short n, void *stream);", ("ebfi_bad", "n")),                 # an unknown scalar type
    ("int ebfi_bad(int n, void (*cb)(int), void *stream);", ("ebfi_bad", "cb")),                # a function pointer
    ("int ebfi_bad(struct ebfi_shape shape, void *stream);", ("ebfi_bad", "shape")),            # a struct by value
    ("int ebfi_bad(const int32_t dims[4], void *stream);", ("ebfi_bad", "dims")),               # an array the rule does not name
    ("int ebfi_bad(int, void *stream);", ("ebfi_bad", "int")),                                  # a parameter without a name
    ("unsigned ebfi_bad(int n);", ("ebfi_bad", "unsigned")),                                    # an unknown return type
    ("int ebfi_bad(int n) { return n; }", ("ebfi_bad",)),                                       # not a prototype
    ("typedef struct { int n; } ebfi_shape;", ("int n",)),
    ("enum { EBFI_SHIFTED = 1 << 2 };", ("EBFI_SHIFTED",)),
])
def test_parser_refuses_what_its_rules_do_not_cover(proto, names):
    with pytest.raises(N.EbfiNativeError) as e:
        N.parse_header("int ebfi_good(int n);\n" + proto + "\n")
    for name in names:
        assert name in str(e.value), str(e.value)


def test_missing_header_is_loud(tmp_path):
    import importlib.util
    import shutil
    copy = tmp_path / "ebfi-be_amd" / "ebfi_amd" / "_native.py"         # a package tree with no include/ beside it
    copy.parent.mkdir(parents=True)
    shutil.copy(N.__file__, copy)
    spec = importlib.util.spec_from_file_location("_native_without_header", str(copy))
    with pytest.raises(RuntimeError) as e:                  # the copy's own EbfiNativeError class
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert type(e.value).__name__ == "EbfiNativeError" and str(tmp_path / "include" / "ebfi_hip.h") in str(e.value)


def test_real_header_rows():
    S = N.SIGNATURES
    assert set(S) == set(N.PARAMS)
    assert S["ebfi_fac_forward"] == (_i, [_vp, _p64, _p64, _vp, _p64, _p64, _i, _vp, _p64, _p64, _i, _vp])
    assert S["ebfi_event_augment"] == (_i, [_vp, _p64, _i64] + [_i] * 8 + [_c.c_uint64, _vp, _i, _i64, _vp, _vp])
    assert S["ebfi_esim_count"] == (_i, [_vp, _p64, _i, _i64, _i, _i, _vp, _vp] + [_c.c_double] * 3 + [_vp, _vp, _vp])
    assert S["ebfi_se_gate_workspace"] == (_c.c_size_t, [_i, _i, _i64])
    assert S["ebfi_last_error"] == (_c.c_char_p, [])
    assert S["ebfi_prof_enable"] == (None, [_i])
    assert N.PARAMS["ebfi_conv2d_forward"][-4:] == ["int act", "float slope", "int dtype", "void *stream"]


def test_constants_come_from_the_header():
    from ebfi_amd import dp, esim, eventaug
    C = N.CONSTANTS
    assert C["EBFI_ABI_VERSION"] == 14 == N.ABI_VERSION
    assert (N.EBFI_F32, N.EBFI_F32_BF16MMA, N.EBFI_F32_BF16X3MMA) == (0, 2, 3) == (C["EBFI_F32"], C["EBFI_F32_BF16MMA"], C["EBFI_F32_BF16X3MMA"])
    assert N.EBFI_ERR_UNSUPPORTED == -3 == C["EBFI_ERR_UNSUPPORTED"]
    assert [C["EBFI_OPTIM_" + k] for k in ("ADAM", "SGD", "DECOUPLED_DECAY", "AMSGRAD", "NESTEROV")] == [0, 1, 1, 2, 4]
    assert (dp._OPTIM_ADAM, dp._OPTIM_SGD, dp._OPTIM_DECOUPLED_DECAY, dp._OPTIM_AMSGRAD, dp._OPTIM_NESTEROV) == (0, 1, 1, 2, 4)
    assert C["EBFI_NOISE_TABLE_MAX"] == 32 == eventaug.TABLE_MAX
    assert C["EBFI_ESIM_MAX_CHUNK"] == 128 == esim.MAX_CHUNK


def test_a_stray_argument_is_refused_with_the_prototype(built_lib):
    lib = N.lib()
    with pytest.raises(TypeError) as e:                     # nothing reaches the library: the count is checked first
        lib.ebfi_conv2d_forward(None, None, None, None, 1, 16, 8, 8, 16, 3, 1, 1, 1, 0.1, 0, 0, None)
    assert "int act, float slope, int dtype, void *stream" in str(e.value) and "16 arguments" in str(e.value)
    for name in ("ebfi_events_workspace", "ebfi_last_error", "ebfi_prof_collect"):
        with pytest.raises(TypeError):
            getattr(lib, name)(*([0] * (len(N.SIGNATURES[name][1]) + 1)))


def test_prof_collect_through_byref_out_parameters(built_lib):
    N.prof_enable(False)
    N.prof_reset()
    assert N.prof_collect() == {"__dropped__": (0, 0.0, 0.0, 0.0)}
