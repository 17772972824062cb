"""The path feddat_head_gemm gives a job (feddat_amd/csrc/head_tail.hip: ht_plan, through feddat_head_gemm_plan) pinned on the CPU:
16-byte or dword loads of A and B, 16-column tiles per wave, and the grid, for every head_gemm call the engines make, every case
of tests/test_head_gemm_kernels_gpu.py, and the edges of each decision.

The choice is invisible to the caller and every path computes the same product, so a moved threshold fails no GPU test by itself:
it moves the tests (and the train step) onto other code paths.  This table is what reports it.  Its values were recorded from
ht_fill as it stood before the decision became a function of its own (the parent's ht_fill, compiled for the host with a main
that prints what it decided), not from the function under test; a row changes only with a reason for the new path."""
import pytest

from feddat_amd import lib
from tests import head_gemm_ref as R

P = R.FAKE_PTRS
FIELDS = ("avec", "bvec", "jt", "itiles", "jblocks", "blocks")


def _job(I, J, K, sa_i, sa_k, sb_k, sb_j, **kw):
    """A feddat_ht_job at made-up addresses, as lib.ht_job fills it (ldo = J unless given)."""
    j = lib.HtJob()
    j.A, j.B, j.out = P["A"], P["B"], P["out"]
    j.I, j.J, j.K, j.sa_i, j.sa_k, j.sb_k, j.sb_j, j.ldo, j.alpha = I, J, K, sa_i, sa_k, sb_k, sb_j, J, 1.0
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def _engine_sites():
    """Every L.ht_job site of vilt_backbone.py (_pool, _head_fwd, _head_bwd), engine.py and vector_engine.py (the pooler backward)
    at H = 768, C = 100, B = 64 and 32; the forward products also at the 2 B rows of the joint P0 + P1 pass; S = 185 tokens."""
    H, C, S = 768, 100, 185
    LN = dict(pro=lib.HT_PRO_LN, pro_a=P["pro_a"], pro_b=P["pro_b"], pro_eps=1e-12, stats_out=P["stats_out"], epi=lib.HT_EPI_TANH,
              bias_j=P["bias_j"])
    out = []
    for nb in (128, 64, 32):
        out += [(f"pool_{nb}", _job(nb, H, H, S * H, 1, 1, H, **LN)),
                (f"fc0_{nb}", _job(nb, 2 * H, H, H, 1, 1, H, bias_j=P["bias_j"])),
                (f"fc1_{nb}", _job(nb, C, 2 * H, 2 * H, 1, 1, 2 * H, bias_j=P["bias_j"])),
                (f"dcls_{nb}", _job(nb, H, H, H, 1, H, 1, pro=lib.HT_PRO_TANH_BWD, pro_a=P["pro_a"], alpha_dev=P["alpha_dev"]))]
    for B in (64, 32):
        out += [(f"dW_fc1_{B}", _job(C, 2 * H, B, 1, C, 2 * H, 1, mode=1, colsum=P["colsum"])),
                (f"dn0_{B}", _job(B, 2 * H, C, C, 1, 2 * H, 1, epi=lib.HT_EPI_MUL_DGELU, aux=P["aux"], ld_aux=2 * H)),
                (f"dW_fc0_{B}", _job(2 * H, H, B, 1, 2 * H, H, 1, mode=1, colsum=P["colsum"])),
                (f"dpooled_{B}", _job(B, H, 2 * H, 2 * H, 1, H, 1))]
    return out


def _edges():
    """The edges of each decision, one change at a time."""
    LN = dict(pro=lib.HT_PRO_LN, pro_a=P["pro_a"], pro_b=P["pro_b"], pro_eps=1e-5)
    out = [
        # 63 | 64 16 x 64 tiles in mode 0 (jt 1 | 4), at 7 x 9 | 8 x 8 and at 4 x 15 | 4 x 16; mode 1 never takes jt 1
        ("tiles_63", _job(112, 576, 64, 64, 1, 1, 64)), ("tiles_64", _job(113, 512, 64, 64, 1, 1, 64)),
        ("tiles_60", _job(49, 960, 64, 64, 1, 1, 64)), ("tiles_64_ragged", _job(49, 961, 64, 64, 1, 1, 64)),
        ("tiles_1_mode1", _job(1, 1, 64, 64, 1, 1, 64, mode=1)),
        # mode 1: eight 64-column groups per block
        ("mode1_J512", _job(16, 512, 32, 1, 16, 512, 1, mode=1)), ("mode1_J513", _job(16, 513, 32, 1, 16, 513, 1, mode=1)),
        # K % 4 in {0, 1}; row strides % 4; each base pointer 4 bytes off
        ("K20", _job(16, 16, 20, 24, 1, 1, 24)), ("K21", _job(16, 16, 21, 24, 1, 1, 24)),
        ("sa_i_25", _job(16, 16, 20, 25, 1, 1, 24)), ("sa_i_26", _job(16, 16, 20, 26, 1, 1, 24)),
        ("sb_j_25", _job(16, 16, 20, 24, 1, 1, 25)), ("sb_j_26", _job(16, 16, 20, 24, 1, 1, 26)),
        ("sa_k_2", _job(16, 16, 20, 40, 2, 1, 24)), ("sb_k_2", _job(16, 16, 20, 24, 1, 2, 40)),
        ("A_off4", _job(16, 16, 20, 24, 1, 1, 24, A=P["A"] + 4)), ("A_off8", _job(16, 16, 20, 24, 1, 1, 24, A=P["A"] + 8)),
        ("B_off4", _job(16, 16, 20, 24, 1, 1, 24, B=P["B"] + 4)), ("A_off16", _job(16, 16, 20, 24, 1, 1, 24, A=P["A"] + 16)),
        ("tanh_bwd_aligned", _job(16, 16, 20, 24, 1, 1, 24, pro=lib.HT_PRO_TANH_BWD, pro_a=P["pro_a"])),
        ("tanh_bwd_y_off4", _job(16, 16, 20, 24, 1, 1, 24, pro=lib.HT_PRO_TANH_BWD, pro_a=P["pro_a"] + 4)),
        ("no_pro_y_off4", _job(16, 16, 20, 24, 1, 1, 24, pro_a=P["pro_a"] + 4)),          # pro_a is not read without a prologue
        ("ln_aligned", _job(16, 16, 20, 24, 1, 1, 24, **LN)),
        ("ln_gamma_off4", _job(16, 16, 20, 24, 1, 1, 24, **dict(LN, pro_a=P["pro_a"] + 4))),
        ("ln_beta_off4", _job(16, 16, 20, 24, 1, 1, 24, **dict(LN, pro_b=P["pro_b"] + 4))),
        ("ln_A_off4", _job(16, 16, 20, 24, 1, 1, 24, A=P["A"] + 4, **LN)),
        ("ln_B_off4", _job(16, 16, 20, 24, 1, 1, 24, B=P["B"] + 4, **LN)),                # B may take dword loads under LN
        ("ln_K2048", _job(16, 16, 2048, 2048, 1, 1, 2048, **LN)), ("ln_K2052", _job(16, 16, 2052, 2052, 1, 1, 2052, **LN)),
        ("ln_K4", _job(16, 16, 4, 4, 1, 1, 4, **LN)),
        ("ldo_eq_J", _job(16, 16, 20, 24, 1, 1, 24, ldo=16)), ("ldo_lt_J", _job(16, 16, 20, 24, 1, 1, 24, ldo=15)),
    ]
    return out


def _refusals():
    out = []
    for name, base, change in R.REFUSALS:
        j = R.fake_job(lib, R.CASE[base])
        change(j)
        out.append(("refuse_" + name, j))
    return out


def all_jobs():
    """(name, job) of everything this file pins, in a fixed order (also what the recording walked)."""
    return ([("site_" + n, j) for n, j in _engine_sites()] + [("edge_" + n, j) for n, j in _edges()] +
            [("case_" + s.name, R.fake_job(lib, s)) for s in R.CASES] + _refusals())


# name -> (avec, bvec, jt, itiles, jblocks, blocks), or None where the entry point answers FEDDAT_EINVAL
EXPECTED = {
    "site_pool_128": (1, 1, 4, 8, 12, 96),
    "site_fc0_128": (1, 1, 4, 8, 24, 192),
    "site_fc1_128": (1, 1, 1, 8, 7, 56),
    "site_dcls_128": (1, 0, 4, 8, 12, 96),
    "site_pool_64": (1, 1, 1, 4, 48, 192),
    "site_fc0_64": (1, 1, 4, 4, 24, 96),
    "site_fc1_64": (1, 1, 1, 4, 7, 28),
    "site_dcls_64": (1, 0, 1, 4, 48, 192),
    "site_pool_32": (1, 1, 1, 2, 48, 96),
    "site_fc0_32": (1, 1, 1, 2, 96, 192),
    "site_fc1_32": (1, 1, 1, 2, 7, 14),
    "site_dcls_32": (1, 0, 1, 2, 48, 96),
    "site_dW_fc1_64": (0, 0, 4, 7, 3, 21),
    "site_dn0_64": (1, 0, 4, 4, 24, 96),
    "site_dW_fc0_64": (0, 0, 4, 96, 2, 192),
    "site_dpooled_64": (1, 0, 1, 4, 48, 192),
    "site_dW_fc1_32": (0, 0, 4, 7, 3, 21),
    "site_dn0_32": (1, 0, 1, 2, 96, 192),
    "site_dW_fc0_32": (0, 0, 4, 96, 2, 192),
    "site_dpooled_32": (1, 0, 1, 2, 48, 96),
    "edge_tiles_63": (1, 1, 1, 7, 36, 252),
    "edge_tiles_64": (1, 1, 4, 8, 8, 64),
    "edge_tiles_60": (1, 1, 1, 4, 60, 240),
    "edge_tiles_64_ragged": (1, 1, 4, 4, 16, 64),
    "edge_tiles_1_mode1": (1, 1, 4, 1, 1, 1),
    "edge_mode1_J512": (0, 0, 4, 1, 1, 1),
    "edge_mode1_J513": (0, 0, 4, 1, 2, 2),
    "edge_K20": (1, 1, 1, 1, 1, 1),
    "edge_K21": (0, 0, 1, 1, 1, 1),
    "edge_sa_i_25": (0, 1, 1, 1, 1, 1),
    "edge_sa_i_26": (0, 1, 1, 1, 1, 1),
    "edge_sb_j_25": (1, 0, 1, 1, 1, 1),
    "edge_sb_j_26": (1, 0, 1, 1, 1, 1),
    "edge_sa_k_2": (0, 1, 1, 1, 1, 1),
    "edge_sb_k_2": (1, 0, 1, 1, 1, 1),
    "edge_A_off4": (0, 1, 1, 1, 1, 1),
    "edge_A_off8": (0, 1, 1, 1, 1, 1),
    "edge_B_off4": (1, 0, 1, 1, 1, 1),
    "edge_A_off16": (1, 1, 1, 1, 1, 1),
    "edge_tanh_bwd_aligned": (1, 1, 1, 1, 1, 1),
    "edge_tanh_bwd_y_off4": (0, 1, 1, 1, 1, 1),
    "edge_no_pro_y_off4": (1, 1, 1, 1, 1, 1),
    "edge_ln_aligned": (1, 1, 1, 1, 1, 1),
    "edge_ln_gamma_off4": None,
    "edge_ln_beta_off4": None,
    "edge_ln_A_off4": None,
    "edge_ln_B_off4": (1, 0, 1, 1, 1, 1),
    "edge_ln_K2048": (1, 1, 1, 1, 1, 1),
    "edge_ln_K2052": None,
    "edge_ln_K4": (1, 1, 1, 1, 1, 1),
    "edge_ldo_eq_J": (1, 1, 1, 1, 1, 1),
    "edge_ldo_lt_J": None,
    "case_a_m0jt1_a1b1_k20": (1, 1, 1, 3, 63, 189),
    "case_a_m0jt1_a1b1_k388": (1, 1, 1, 3, 63, 189),
    "case_a_m0jt1_a1b0_k20": (1, 0, 1, 3, 63, 189),
    "case_a_m0jt1_a1b0_k388": (1, 0, 1, 3, 63, 189),
    "case_a_m0jt1_a0b1_k20": (0, 1, 1, 3, 63, 189),
    "case_a_m0jt1_a0b1_k388": (0, 1, 1, 3, 63, 189),
    "case_a_m0jt1_a0b0_k3": (0, 0, 1, 3, 63, 189),
    "case_a_m0jt1_a0b0_k20": (0, 0, 1, 3, 63, 189),
    "case_a_m0jt1_a0b0_k37": (0, 0, 1, 3, 63, 189),
    "case_a_m0jt1_a0b0_k388": (0, 0, 1, 3, 63, 189),
    "case_a_m0jt4_a1b1_k20": (1, 1, 4, 4, 16, 64),
    "case_a_m0jt4_a1b1_k388": (1, 1, 4, 4, 16, 64),
    "case_a_m0jt4_a1b0_k20": (1, 0, 4, 4, 16, 64),
    "case_a_m0jt4_a1b0_k388": (1, 0, 4, 4, 16, 64),
    "case_a_m0jt4_a0b1_k20": (0, 1, 4, 4, 16, 64),
    "case_a_m0jt4_a0b1_k388": (0, 1, 4, 4, 16, 64),
    "case_a_m0jt4_a0b0_k3": (0, 0, 4, 4, 16, 64),
    "case_a_m0jt4_a0b0_k20": (0, 0, 4, 4, 16, 64),
    "case_a_m0jt4_a0b0_k37": (0, 0, 4, 4, 16, 64),
    "case_a_m0jt4_a0b0_k388": (0, 0, 4, 4, 16, 64),
    "case_a_m1_a1b1_k20": (1, 1, 4, 4, 2, 8),
    "case_a_m1_a1b1_k388": (1, 1, 4, 4, 2, 8),
    "case_a_m1_a1b0_k20": (1, 0, 4, 4, 2, 8),
    "case_a_m1_a1b0_k388": (1, 0, 4, 4, 2, 8),
    "case_a_m1_a0b1_k20": (0, 1, 4, 4, 2, 8),
    "case_a_m1_a0b1_k388": (0, 1, 4, 4, 2, 8),
    "case_a_m1_a0b0_k3": (0, 0, 4, 4, 2, 8),
    "case_a_m1_a0b0_k20": (0, 0, 4, 4, 2, 8),
    "case_a_m1_a0b0_k37": (0, 0, 4, 4, 2, 8),
    "case_a_m1_a0b0_k388": (0, 0, 4, 4, 2, 8),
    "case_b_m0jt1_Aoff": (0, 1, 1, 3, 63, 189),
    "case_b_m0jt1_Boff": (1, 0, 1, 3, 63, 189),
    "case_b_m0jt4_Aoff": (0, 1, 4, 4, 16, 64),
    "case_b_m0jt4_Boff": (1, 0, 4, 4, 16, 64),
    "case_b_m1_Aoff": (0, 1, 4, 4, 2, 8),
    "case_b_m1_Boff": (1, 0, 4, 4, 2, 8),
    "case_b_m0jt4_Astride": (0, 1, 4, 4, 16, 64),
    "case_b_m0jt4_Bstride": (1, 0, 4, 4, 16, 64),
    "case_c_rows16_a1b1": (1, 1, 1, 1, 63, 63),
    "case_c_rows16_a0b0": (0, 0, 1, 1, 63, 63),
    "case_d_k772_i64_bv_jt4_stats": (1, 1, 4, 4, 16, 64),
    "case_d_k2048_i17_bd_jt1": (1, 0, 1, 2, 7, 14),
    "case_d_k4_i1_bv_jt1_stats": (1, 1, 1, 1, 3, 3),
    "case_d_k4_i17_bd_jt4_stats": (1, 0, 4, 2, 32, 64),
    "case_d_k772_i17_bv_m1_stats": (1, 1, 4, 2, 2, 4),
    "case_d_k4_i64_bd_m1": (1, 0, 4, 4, 1, 4),
    "case_d_k2048_i1_bv_jt1_stats": (1, 1, 1, 1, 7, 7),
    "case_d_k4_i17_shift1000": (1, 1, 1, 2, 7, 14),
    "case_d_k4_i17_shift1000_m1": (1, 0, 4, 2, 1, 2),
    "case_e_vec_m0jt4": (1, 0, 4, 4, 16, 64),
    "case_e_vec_m0jt1": (1, 1, 1, 3, 7, 21),
    "case_e_dw_m0jt1": (0, 0, 1, 3, 7, 21),
    "case_e_dw_m0jt4": (0, 1, 4, 4, 16, 64),
    "case_e_vec_m1": (1, 0, 4, 4, 1, 4),
    "case_e_dw_m1": (0, 0, 4, 4, 1, 4),
    "case_e_yoff_m0jt4": (0, 0, 4, 4, 16, 64),
    "case_e_yoff_m1": (0, 0, 4, 4, 1, 4),
    "case_f_tanh_jt1": (1, 1, 1, 2, 7, 14),
    "case_f_tanh_jt4": (0, 0, 4, 4, 16, 64),
    "case_f_tanh_m1": (1, 1, 4, 2, 1, 2),
    "case_f_dgelu_jt1": (0, 0, 1, 2, 7, 14),
    "case_f_dgelu_jt4": (1, 0, 4, 4, 16, 64),
    "case_f_dgelu_m1": (0, 1, 4, 2, 1, 2),
    "case_f_bias_alpha_jt1": (1, 1, 1, 2, 4, 8),
    "case_g_cs_one_block": (0, 0, 1, 2, 1, 2),
    "case_g_cs_jt1": (1, 1, 1, 2, 13, 26),
    "case_g_cs_jt1_dw": (0, 0, 1, 2, 13, 26),
    "case_g_cs_jt4": (1, 0, 4, 4, 16, 64),
    "case_j_pool": (1, 1, 1, 4, 48, 192),
    "case_j_fc0": (1, 1, 4, 4, 24, 96),
    "case_j_fc1": (1, 1, 1, 4, 7, 28),
    "case_j_dW_fc1": (0, 0, 4, 7, 3, 21),
    "case_j_dn0": (1, 0, 4, 4, 24, 96),
    "case_j_dW_fc0": (0, 0, 4, 96, 2, 192),
    "case_j_dpooled": (1, 0, 1, 4, 48, 192),
    "case_j_dcls": (1, 0, 1, 4, 48, 192),
    "case_i_plain": (1, 1, 1, 2, 3, 6),
    "case_i_ln": (1, 1, 1, 2, 3, 6),
    "case_i_tb": (1, 1, 1, 2, 3, 6),
    "case_i_dg": (1, 1, 1, 2, 3, 6),
    "refuse_I_0": None,
    "refuse_J_0": None,
    "refuse_K_0": None,
    "refuse_I_negative": None,
    "refuse_A_null": None,
    "refuse_B_null": None,
    "refuse_out_null": None,
    "refuse_ldo_lt_J": None,
    "refuse_mode_2": None,
    "refuse_mode_negative": None,
    "refuse_pro_3": None,
    "refuse_pro_negative": None,
    "refuse_epi_3": None,
    "refuse_epi_negative": None,
    "refuse_ln_K_mod_4": None,
    "refuse_ln_K_gt_2048": None,
    "refuse_ln_sa_k_2": None,
    "refuse_ln_sa_i_mod_4": None,
    "refuse_ln_eps_0": None,
    "refuse_ln_eps_negative": None,
    "refuse_ln_A_misaligned": None,
    "refuse_ln_gamma_misaligned": None,
    "refuse_ln_beta_misaligned": None,
    "refuse_ln_gamma_null": None,
    "refuse_ln_beta_null": None,
    "refuse_tanh_bwd_y_null": None,
    "refuse_dgelu_aux_null": None,
    "refuse_dgelu_ld_aux_lt_J": None,
}


@pytest.fixture(params=["bf16", "f16"])
def operands(request):
    with lib.operands(request.param):
        yield request.param


def test_plans_match_the_recorded_table(operands):
    jobs = all_jobs()
    assert sorted(n for n, _ in jobs) == sorted(EXPECTED), "every pinned job has a recorded row and the other way round"
    for name, j in jobs:
        want = EXPECTED[name]
        if want is None:
            with pytest.raises(lib.FeddatHipError, match="EINVAL"):
                lib.head_gemm_plan(j)
            continue
        p = lib.head_gemm_plan(j)
        assert tuple(p[f] for f in FIELDS) == want, name


def test_gpu_cases_take_the_path_they_are_there_for(operands):
    """Each case of the GPU file names the (avec, bvec, jt) it is there to exercise; the GPU test asserts it before it launches, and
    here the same claim is held against the RECORDED table, so it does not rest on the function under test."""
    for s in R.CASES:
        assert EXPECTED["case_" + s.name][:3] == s.want, s.name
    for name, base, _ in R.REFUSALS:
        assert EXPECTED["refuse_" + name] is None and EXPECTED["case_" + base] is not None, name


def test_plan_claims_of_the_comments(operands):
    """What head_tail.hip and the issue trail say in prose about where the step's products run."""
    e = EXPECTED
    # fc0 at 64 x 1536 x 768 runs on 96 16 x 64 tiles; fc1 (64 x 100) and d(pooled) (32 x 768) are the few-tile products on 16 x 16
    assert e["site_fc0_64"] == (1, 1, 4, 4, 24, 96) and e["site_fc1_64"][2] == 1 and e["site_dpooled_32"][2] == 1
    # at 64 rows the pooler and its backward run on 16 x 16 tiles (48 tiles of 16 x 64), at 128 rows on 16 x 64 (96)
    assert e["site_pool_64"][2] == e["site_dcls_64"][2] == 1 and e["site_pool_128"][2] == e["site_dcls_128"][2] == 4
    # a [J, K] row-major weight is fetched with 16-byte loads, the transposed use of the same weight with dword loads
    assert e["site_pool_64"][:2] == (1, 1) and e["site_dcls_64"][:2] == (1, 0)
    # the batch contractions (mode 1) read both operands across k with dword loads
    assert all(e[f"site_{n}_{B}"][:3] == (0, 0, 4) for n in ("dW_fc1", "dW_fc0") for B in (64, 32))
    # the plan needs nothing but the job: no pointer is dereferenced (all of them are made up) and NULL out is refused
    assert lib.load().feddat_head_gemm_plan(None, None) == 1
