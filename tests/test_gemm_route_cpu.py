"""The GEMM routing (feddat_amd/csrc/gemm_route.h through feddat_gemm_route) pinned on the CPU: which kernel family, tile height,
grid, LDS size and XCD split every production shape, every edge and every selection flag gets on a 256-CU device.

Every kernel variant is bit-identical to the others (test_ops_gpu.py::test_gemm_kernel_variants_bit_identical), so a routing
mistake fails no GPU test -- it only makes the step slower.  This table is what reports it.  Its values were recorded from the
routing as it stood before it became one function (launches replaced by recording), not from the function under test; a row
changes only with a measurement that justifies the new route."""
import pytest

from feddat_amd import lib
from feddat_amd.lib import GEMM_DUAL as DUAL, GEMM_FP8 as FP8, GEMM_FP8MX as FP8MX, GEMM_MID as MID, GEMM_OP16 as OP16
from feddat_amd.lib import GEMM_V1 as V1, GEMM_V2 as V2, GEMM_V3 as V3

N_CU = 256
FIELDS = ("family", "rows", "grid", "lds_bytes", "bm", "tiles_m", "nx", "tm_per", "tn_per")
# (kind, M, N, K, epilogues, flags, expected): expected = FIELDS, or None where the entry point answers FEDDAT_EINVAL.
# Epilogues: 0 BF16, 1 RESID_F32, 2 GELU, 3 MUL_DGELU, 4 F32, 5 GELU_G8, 6 MUL_G8, 7 GELU_G8_F8, 8 MUL_G8_F8.
ROUTES = [
    # ---- the production shapes of bench.py's ViLT (M = 11840 / 5920) and ALBEF (18464 / 4608 / 1600) workloads, every epilogue
    (OP16, 11840, 2304, 768, (0, 1, 4), 0, (V3, 192, 256, 118784, 185, 64, 2, 16, 6)),
    (OP16, 11840, 2304, 768, (2, 3, 5, 6), 0, (V2, 192, 256, 139264, 185, 64, 2, 16, 6)),
    (OP16, 11840, 768, 768, (0, 1, 4), 0, (V3, 192, 248, 118784, 191, 62, 1, 7, 4)),
    (OP16, 11840, 768, 768, (2, 3, 5, 6), 0, (V2, 192, 248, 139264, 191, 62, 1, 7, 4)),
    (OP16, 11840, 3072, 768, (0, 1, 4), 0, (V3, 256, 256, 135168, 247, 48, 2, 12, 8)),
    (OP16, 11840, 3072, 768, (2, 5, 6), 0, (V2, 256, 256, 155648, 247, 48, 2, 12, 8)),
    (OP16, 11840, 3072, 768, (3,), 0, (V2, 192, 256, 139264, 185, 64, 2, 16, 8)),
    (OP16, 11840, 768, 3072, (0, 1, 4), 0, (V3, 192, 248, 118784, 191, 62, 1, 7, 4)),
    (OP16, 11840, 768, 3072, (2, 3, 5, 6), 0, (V2, 192, 248, 139264, 191, 62, 1, 7, 4)),
    (OP16, 5920, 2304, 768, (0, 1, 4), 0, (V3, 160, 256, 110592, 148, 40, 2, 10, 6)),
    (OP16, 5920, 2304, 768, (2, 3, 5, 6), 0, (V2, 192, 256, 139264, 185, 32, 2, 8, 6)),
    (OP16, 5920, 768, 768, (0, 1, 4), 0, (V3, 160, 148, 110592, 160, 37, 1, 4, 4)),
    (OP16, 5920, 768, 768, (2, 3, 5, 6), 0, (V2, 192, 124, 139264, 191, 31, 1, 3, 4)),
    (OP16, 5920, 3072, 768, (0, 1, 4), 0, (V3, 192, 256, 118784, 185, 32, 2, 8, 8)),
    (OP16, 5920, 3072, 768, (2, 3, 5, 6), 0, (V2, 192, 256, 139264, 185, 32, 2, 8, 8)),
    (OP16, 5920, 768, 3072, (0, 1, 4), 0, (V3, 160, 148, 110592, 160, 37, 1, 4, 4)),
    (OP16, 5920, 768, 3072, (2, 3, 5, 6), 0, (V2, 192, 124, 139264, 191, 31, 1, 3, 4)),
    (OP16, 18464, 768, 768, (0, 1, 4), 0, (V3, 160, 256, 110592, 160, 116, 1, 14, 4)),
    (OP16, 18464, 768, 768, (2, 3, 5, 6), 0, (V2, 192, 256, 139264, 191, 97, 1, 12, 4)),
    (OP16, 18464, 2304, 768, (0, 1, 4), 0, (V3, 224, 256, 126976, 220, 84, 2, 21, 6)),
    (OP16, 18464, 2304, 768, (2, 5, 6), 0, (V2, 256, 256, 155648, 243, 76, 2, 19, 6)),
    (OP16, 18464, 2304, 768, (3,), 0, (V2, 192, 256, 139264, 185, 100, 2, 25, 6)),
    (OP16, 18464, 3072, 768, (0, 1, 4), 0, (V3, 256, 256, 135168, 243, 76, 2, 19, 8)),
    (OP16, 18464, 3072, 768, (2, 5, 6), 0, (V2, 256, 256, 155648, 243, 76, 2, 19, 8)),
    (OP16, 18464, 3072, 768, (3,), 0, (V2, 192, 256, 139264, 185, 100, 2, 25, 8)),
    (OP16, 18464, 768, 3072, (0, 1, 4), 0, (V3, 160, 256, 110592, 160, 116, 2, 29, 2)),
    (OP16, 18464, 768, 3072, (2, 3, 5, 6), 0, (V2, 192, 256, 139264, 185, 100, 2, 25, 2)),
    (OP16, 4608, 768, 3072, (0, 1, 4), 0, (V3, 160, 116, 110592, 159, 29, 1, 3, 4)),
    (OP16, 4608, 768, 3072, (2, 3, 5, 6), 0, (V2, 192, 96, 139264, 192, 24, 1, 3, 4)),
    (OP16, 1600, 768, 768, (0, 1, 2, 3, 4), 0, (MID, 64, 300, 32768, 0, 0, 0, 0, 0)),
    (OP16, 1600, 768, 768, (5, 6), 0, (V2, 192, 36, 139264, 178, 9, 1, 1, 4)),
    (OP16, 1600, 2304, 768, (0, 1, 2, 3, 4), 0, (V1, 128, 234, 65536, 0, 0, 0, 0, 0)),
    (OP16, 1600, 2304, 768, (5, 6), 0, (V2, 192, 108, 139264, 178, 9, 1, 1, 12)),
    (OP16, 1600, 3072, 768, (0, 1, 2, 3, 4), 0, (V1, 128, 312, 65536, 0, 0, 0, 0, 0)),
    (OP16, 1600, 3072, 768, (5, 6), 0, (V2, 192, 144, 139264, 178, 9, 1, 1, 16)),
    (OP16, 1600, 768, 3072, (0, 1, 2, 3, 4), 0, (MID, 64, 300, 32768, 0, 0, 0, 0, 0)),
    (OP16, 1600, 768, 3072, (5, 6), 0, (V2, 192, 36, 139264, 178, 9, 1, 1, 4)),
    # ---- edges, at the smallest shapes that reach them: M = 1023 / 1024; the small-grid rule at M = 4095 / 4096; N % 192 != 0;
    # N = 192 x 3 with and without flag 128; code epilogues below 1024 rows / off the persistent kernels / with flag 2; bad shapes
    (OP16, 1023, 192, 64, (0, 1, 2, 3, 4), 0, (MID, 64, 48, 32768, 0, 0, 0, 0, 0)),
    (OP16, 1023, 192, 64, (5, 6), 0, None),
    (OP16, 1024, 192, 64, (0, 1, 2, 3, 4), 0, (MID, 64, 48, 32768, 0, 0, 0, 0, 0)),
    (OP16, 1024, 192, 64, (5, 6), 0, (V2, 192, 6, 139264, 171, 6, 1, 0, 1)),
    (OP16, 4095, 768, 768, (0, 1, 2, 3, 4), 0, (V1, 128, 192, 65536, 0, 0, 0, 0, 0)),
    (OP16, 4095, 768, 768, (5, 6), 0, (V2, 192, 88, 139264, 187, 22, 1, 2, 4)),
    (OP16, 4096, 768, 768, (0, 1, 4), 0, (V3, 160, 104, 110592, 158, 26, 1, 3, 4)),
    (OP16, 4096, 768, 768, (2, 3, 5, 6), 0, (V2, 192, 88, 139264, 187, 22, 1, 2, 4)),
    (OP16, 1200, 256, 192, (0, 1, 2, 3, 4), 0, (V1, 128, 20, 65536, 0, 0, 0, 0, 0)),
    (OP16, 1200, 256, 192, (5, 6), 0, None),
    (OP16, 1030, 640, 64, (0, 1, 2, 3, 4), 0, (V1, 128, 45, 65536, 0, 0, 0, 0, 0)),
    (OP16, 1030, 640, 64, (5, 6), 0, None),
    (OP16, 1030, 576, 64, (0, 1, 2, 3, 4), 0, (MID, 64, 153, 32768, 0, 0, 0, 0, 0)),
    (OP16, 1030, 576, 64, (5, 6), 0, (V2, 192, 18, 139264, 172, 6, 1, 0, 3)),
    (OP16, 1030, 576, 64, (0, 1, 4), 128, (V3, 160, 21, 110592, 148, 7, 1, 0, 3)),
    (OP16, 1030, 576, 64, (2, 3, 5, 6), 128, (V2, 192, 18, 139264, 172, 6, 1, 0, 3)),
    (OP16, 1030, 192, 64, (0, 1, 2, 3, 4), 0, (MID, 64, 51, 32768, 0, 0, 0, 0, 0)),
    (OP16, 1030, 192, 64, (5, 6), 0, (V2, 192, 6, 139264, 172, 6, 1, 0, 1)),
    (OP16, 2051, 384, 192, (0, 1, 2, 3, 4), 0, (MID, 64, 198, 32768, 0, 0, 0, 0, 0)),
    (OP16, 2051, 384, 192, (5, 6), 0, (V2, 192, 22, 139264, 187, 11, 1, 1, 2)),
    (OP16, 1000, 768, 768, (5, 6), 0, None),
    (OP16, 11840, 3072, 768, (5, 6), 2, None),
    (OP16, 8, 100, 60, (0,), 0, None),
    (OP16, 1200, 200, 192, (0,), 0, None),
    # ---- every selection flag of test_gemm_kernel_variants_bit_identical; flags 3 at K = 128 (two k-tiles: the dual form is not
    # taken and the route is the production one, listed next to it); the grid cap 2 << 28
    (OP16, 11840, 3072, 768, (0, 1, 2, 3, 4, 5, 6), 33, (V2, 192, 256, 139264, 185, 64, 2, 16, 8)),
    (OP16, 11840, 3072, 768, (0, 1, 2, 3, 4, 5, 6), 65, (V2, 256, 256, 155648, 247, 48, 2, 12, 8)),
    (OP16, 11840, 3072, 768, (0, 1, 2, 3, 4), 34, (V3, 192, 256, 118784, 185, 64, 2, 16, 8)),
    (OP16, 11840, 3072, 768, (5, 6), 34, None),
    (OP16, 11840, 3072, 768, (0, 1, 2, 3, 4), 66, (V3, 256, 256, 135168, 247, 48, 2, 12, 8)),
    (OP16, 11840, 3072, 768, (5, 6), 66, None),
    (OP16, 11840, 3072, 768, (0, 1, 2, 4), 2, (V3, 256, 256, 135168, 247, 48, 2, 12, 8)),
    (OP16, 11840, 3072, 768, (3,), 2, (V3, 192, 256, 118784, 185, 64, 2, 16, 8)),
    (OP16, 11840, 3072, 768, (5, 6), 2, None),
    (OP16, 11840, 3072, 768, (0, 1, 4), 0x8000000, (V3, 256, 256, 135168, 247, 48, 2, 12, 8)),
    (OP16, 11840, 3072, 768, (2, 5, 6), 0x8000000, (V2, 256, 256, 155648, 247, 48, 2, 12, 8)),
    (OP16, 11840, 3072, 768, (3,), 0x8000000, (V2, 192, 256, 139264, 185, 64, 2, 16, 8)),
    (OP16, 11840, 3072, 768, (0, 1, 2, 3, 4, 5, 6), 3, (DUAL, 128, 512, 81920, 124, 96, 2, 24, 8)),
    (OP16, 11840, 3072, 768, (0, 1, 2, 3, 4, 5, 6), 67, (DUAL, 128, 512, 81920, 124, 96, 2, 24, 8)),
    (OP16, 5920, 2304, 768, (0, 1, 2, 3, 4, 5, 6), 33, (V2, 192, 256, 139264, 185, 32, 2, 8, 6)),
    (OP16, 5920, 2304, 768, (0, 1, 2, 3, 4, 5, 6), 65, (V2, 256, 256, 155648, 247, 24, 2, 6, 6)),
    (OP16, 5920, 2304, 768, (0, 1, 2, 3, 4), 34, (V3, 192, 256, 118784, 185, 32, 2, 8, 6)),
    (OP16, 5920, 2304, 768, (5, 6), 34, None),
    (OP16, 5920, 2304, 768, (0, 1, 2, 3, 4), 66, (V3, 256, 256, 135168, 247, 24, 2, 6, 6)),
    (OP16, 5920, 2304, 768, (5, 6), 66, None),
    (OP16, 5920, 2304, 768, (0, 1, 2, 3, 4), 2, (V3, 160, 256, 110592, 148, 40, 2, 10, 6)),
    (OP16, 5920, 2304, 768, (5, 6), 2, None),
    (OP16, 5920, 2304, 768, (0, 1, 4), 0x8000000, (V3, 192, 256, 118784, 185, 32, 2, 8, 6)),
    (OP16, 5920, 2304, 768, (2, 3, 5, 6), 0x8000000, (V2, 192, 256, 139264, 185, 32, 2, 8, 6)),
    (OP16, 5920, 2304, 768, (0, 1, 2, 3, 4, 5, 6), 3, (DUAL, 128, 512, 81920, 124, 48, 2, 12, 6)),
    (OP16, 5920, 2304, 768, (0, 1, 4), 67, (V3, 256, 256, 135168, 247, 24, 2, 6, 6)),
    (OP16, 5920, 2304, 768, (2, 3, 5, 6), 67, (V2, 256, 256, 155648, 247, 24, 2, 6, 6)),
    (OP16, 11840, 3072, 128, (0, 1, 4), 3, (V3, 256, 256, 135168, 252, 47, 1, 5, 16)),
    (OP16, 11840, 3072, 128, (2, 5, 6), 3, (V2, 256, 256, 155648, 252, 47, 1, 5, 16)),
    (OP16, 11840, 3072, 128, (3,), 3, (V2, 192, 256, 139264, 191, 62, 1, 7, 16)),
    (OP16, 11840, 3072, 128, (0, 1, 4), 0, (V3, 256, 256, 135168, 252, 47, 1, 5, 16)),
    (OP16, 11840, 3072, 128, (2, 5, 6), 0, (V2, 256, 256, 155648, 252, 47, 1, 5, 16)),
    (OP16, 11840, 3072, 128, (3,), 0, (V2, 192, 256, 139264, 191, 62, 1, 7, 16)),
    (OP16, 11840, 3072, 768, (0, 1, 4), 0x20000000, (V3, 256, 32, 135168, 247, 48, 2, 12, 8)),
    (OP16, 11840, 3072, 768, (2, 5, 6), 0x20000000, (V2, 256, 32, 155648, 247, 48, 2, 12, 8)),
    (OP16, 11840, 3072, 768, (3,), 0x20000000, (V2, 192, 32, 139264, 185, 64, 2, 16, 8)),
    (OP16, 11840, 3072, 768, (0, 1, 2, 3, 4, 5, 6), 0x20000003, (DUAL, 128, 64, 81920, 124, 96, 2, 24, 8)),
    (OP16, 5920, 2304, 128, (0, 1, 4), 3, (V3, 160, 256, 110592, 160, 37, 1, 4, 12)),
    (OP16, 5920, 2304, 128, (2, 3, 5, 6), 3, (V2, 192, 256, 139264, 191, 31, 1, 3, 12)),
    (OP16, 5920, 2304, 128, (0, 1, 4), 0, (V3, 160, 256, 110592, 160, 37, 1, 4, 12)),
    (OP16, 5920, 2304, 128, (2, 3, 5, 6), 0, (V2, 192, 256, 139264, 191, 31, 1, 3, 12)),
    (OP16, 5920, 2304, 768, (0, 1, 4), 0x20000000, (V3, 256, 32, 135168, 247, 24, 2, 6, 6)),
    (OP16, 5920, 2304, 768, (2, 5, 6), 0x20000000, (V2, 256, 32, 155648, 247, 24, 2, 6, 6)),
    (OP16, 5920, 2304, 768, (3,), 0x20000000, (V2, 192, 32, 139264, 185, 32, 2, 8, 6)),
    (OP16, 5920, 2304, 768, (0, 1, 2, 3, 4, 5, 6), 0x20000003, (DUAL, 128, 64, 81920, 124, 48, 2, 12, 6)),
    # ---- fp8 operands: . gelu'(bf16 u) (3,) and the residual epilogue (1,) never take 256 rows; MX: + the scale stages; flag 256
    (FP8, 11840, 2304, 768, (0, 1, 2, 3, 4, 5, 6, 7, 8), 0, (V2, 192, 256, 139264, 191, 62, 1, 7, 12)),
    (FP8, 11840, 2304, 768, (0, 1, 2, 3, 4, 5, 6, 7, 8), 0x100, (V2, 192, 256, 139264, 191, 62, 1, 7, 12)),
    (FP8MX, 11840, 2304, 768, (0,), 0, (V2, 192, 256, 140800, 191, 62, 1, 7, 12)),
    (FP8, 11840, 3072, 768, (0, 2, 4, 5, 6, 7, 8), 0, (V2, 256, 256, 155648, 252, 47, 1, 5, 16)),
    (FP8, 11840, 3072, 768, (1, 3), 0, (V2, 192, 256, 139264, 191, 62, 1, 7, 16)),
    (FP8, 11840, 3072, 768, (0, 2, 4, 5, 6, 7, 8), 0x100, (V2, 256, 256, 155648, 252, 47, 1, 5, 16)),
    (FP8, 11840, 3072, 768, (1, 3), 0x100, (V2, 192, 256, 139264, 191, 62, 1, 7, 16)),
    (FP8MX, 11840, 3072, 768, (0,), 0, (V2, 256, 256, 157696, 252, 47, 1, 5, 16)),
    (FP8, 1000, 768, 768, (0,), 0, None),
    (FP8, 11840, 768, 64, (0,), 0, None),
]


@pytest.fixture(params=["bf16", "f16"])
def operands(request):
    with lib.operands(request.param):
        yield request.param


def _route(kind, M, N, K, epi, flags=0):
    return lib.gemm_route(M, N, K, epi, kind=kind, n_cu=N_CU, flags=flags)


def test_routes_match_the_recorded_table(operands):
    for kind, M, N, K, epis, flags, want in ROUTES:
        for epi in epis:
            case = (kind, M, N, K, epi, hex(flags))
            if want is None:
                with pytest.raises(lib.FeddatHipError, match="EINVAL"):
                    _route(kind, M, N, K, epi, flags)
                continue
            r = _route(kind, M, N, K, epi, flags)
            assert tuple(r[f] for f in FIELDS) == want, case
            assert r["threads"] == (512 if r["family"] == V2 else 256), case


def test_routing_claims_of_the_comments(operands):
    """What the source and test_ops_gpu.py say in prose about where the production shapes run."""
    light, heavy = (lib.EPI_BF16, lib.EPI_RESID_F32, lib.EPI_F32), (lib.EPI_GELU, lib.EPI_MUL_DGELU, lib.EPI_GELU_G8, lib.EPI_MUL_G8)
    vilt = [(M, N, K) for M in (11840, 5920) for N, K in ((2304, 768), (768, 768), (3072, 768), (768, 3072))]
    albef = [(18464, 768, 768), (18464, 2304, 768), (18464, 3072, 768), (18464, 768, 3072), (4608, 768, 3072)]
    # GELU, . gelu' and the code epilogues are on the two-group kernel, everything else on one wave per SIMD
    for M, N, K in vilt + albef:
        assert {_route(OP16, M, N, K, e)["family"] for e in light} == {V3}, (M, N, K)
        assert {_route(OP16, M, N, K, e)["family"] for e in heavy} == {V2}, (M, N, K)
    # 11840 x 3072 x 768 is the one ViLT shape on 256-row tiles (ALBEF's 18464 rows take them at N = 3072 too, and the two-group
    # kernel at N = 2304); . gelu'(bf16 u) never does
    on256 = {s for s in vilt + albef for e in light + heavy if _route(OP16, *s, e)["rows"] == 256}
    assert on256 == {(11840, 3072, 768), (18464, 3072, 768), (18464, 2304, 768)}
    assert {_route(OP16, 18464, 2304, 768, e)["rows"] for e in light} == {224}
    assert all(_route(OP16, *s, lib.EPI_MUL_DGELU)["rows"] == 192 for s in vilt + albef)
    # 160-row tiles where they fill the rounds better
    for s in ((5920, 2304, 768), (18464, 768, 768), (5920, 768, 3072), (4608, 768, 3072), (5920, 768, 768)):
        assert {_route(OP16, *s, e)["rows"] for e in light} == {160}, s
    # ALBEF's stacked text streams: 1600 x 768 goes to the small-tile kernel, except with the code epilogues
    for K in (768, 3072):
        assert {_route(OP16, 1600, 768, K, e)["family"] for e in range(5)} == {MID}
        assert {_route(OP16, 1600, 768, K, e)["family"] for e in (lib.EPI_GELU_G8, lib.EPI_MUL_G8)} == {V2}
    # flag 128: N = 192 x 3 stays persistent instead of losing its tail columns on the 128 x 128 kernel
    assert _route(OP16, 1030, 576, 64, lib.EPI_BF16)["family"] == MID
    assert _route(OP16, 1030, 576, 64, lib.EPI_BF16, 128)["family"] == V3
    # flags 3 with two k-tiles: the dual form is not taken, the kernel sees the flags without them
    assert _route(OP16, 11840, 3072, 128, lib.EPI_BF16, 3) == _route(OP16, 11840, 3072, 128, lib.EPI_BF16, 0)
    assert _route(OP16, 11840, 3072, 768, lib.EPI_BF16, 3)["dbg"] == 3 and _route(FP8, 11840, 3072, 768, lib.EPI_BF16, 256)["dbg"] == 0


def test_every_route_covers_the_product(operands):
    """Over a grid of shapes: the grid fits the device, the tiles are no higher than the kernel's and cover M, and the 4 x 2 XCD
    split divides the tiles evenly."""
    for M in range(1024, 20001, 97):
        for N in (192, 768, 2304, 3072):
            for K in (64, 768, 3072):
                for flags in (0, 3):
                    for epi in (lib.EPI_BF16, lib.EPI_GELU, lib.EPI_MUL_DGELU, lib.EPI_GELU_G8):      # one of each routing class
                        r = _route(OP16, M, N, K, epi, flags)
                        case = (M, N, K, epi, flags, r)
                        if r["family"] in (V1, MID):
                            assert M < 4096 and epi < 5, case
                            continue
                        assert (r["family"] == DUAL) == (flags == 3 and K >= 192), case
                        assert 0 < r["grid"] <= (2 * N_CU if r["family"] == DUAL else N_CU), case
                        assert r["grid"] <= r["tiles_m"] * (N // 192), case
                        assert 0 < r["bm"] <= r["rows"] and r["bm"] * r["tiles_m"] >= M, case
                        assert r["nx"] in (1, 2), case
                        if r["nx"] == 2:
                            assert r["tm_per"] * 4 == r["tiles_m"] and r["tn_per"] * 2 == N // 192, case
