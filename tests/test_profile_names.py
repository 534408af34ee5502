"""Kernel symbol -> profile name (scripts/collect_traffic_names.py, shared by the profile reducers): the pointwise kernel's
symbols, as the committed traces carry them (two kernels) and as the library has them now (one kernel <KS, NBW>), and one
symbol of every other family the function knows."""
import importlib.util
import os

import pytest

_spec = importlib.util.spec_from_file_location("collect_traffic_names", os.path.join(os.path.dirname(__file__), "..", "scripts", "collect_traffic_names.py"))
_names = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_names)

POINTWISE = [
    # the single kernel: NBW = 1 is the single-block form
    ("void irmv::conv1x1_pw_kernel<4, 1>(irmv::ConvArgs, int)", "conv1x1s1_pw"),
    ("void irmv::conv1x1_pw_kernel<16, 1>(irmv::ConvArgs, int)", "conv1x1s1_pw"),
    ("void irmv::conv1x1_pw_kernel<12, 2>(irmv::ConvArgs, int)", "conv1x1s1_pw_n2"),
    ("void irmv::conv1x1_pw_kernel<8, 4>(irmv::ConvArgs, int)", "conv1x1s1_pw_n4"),
    ("_ZN4irmv17conv1x1_pw_kernelILi6ELi1EEEvNS_8ConvArgsEi", "conv1x1s1_pw"),
    ("_ZN4irmv17conv1x1_pw_kernelILi12ELi2EEEvNS_8ConvArgsEi", "conv1x1s1_pw_n2"),
    ("_ZN4irmv17conv1x1_pw_kernelILi4ELi4EEEvNS_8ConvArgsEi", "conv1x1s1_pw_n4"),
    # the two kernels of the committed traces
    ("void irmv::conv1x1_pw_kernel<4>(irmv::ConvArgs, int, int)", "conv1x1s1_pw"),
    ("_ZN4irmv17conv1x1_pw_kernelILi8EEEvNS_8ConvArgsEii", "conv1x1s1_pw"),
    ("void irmv::conv1x1_pwn_kernel<12, 2>(irmv::ConvArgs, int)", "conv1x1s1_pw_n2"),
    ("void irmv::conv1x1_pwn_kernel<8, 4>(irmv::ConvArgs, int)", "conv1x1s1_pw_n4"),
    ("_ZN4irmv18conv1x1_pwn_kernelILi16ELi2EEEvNS_8ConvArgsEi", "conv1x1s1_pw_n2"),
]

OTHERS = [
    ("_ZN4irmv18conv3x3_lds_kernelILi1ELi2ELi4ELb0ELi0ELi0ELi0ELi4ELi0ELb0EEEvNS_8ConvArgsEPKDF16_iiiiiiii", "conv3x3s1_lds_mt2_nt4"),
    ("_ZN4irmv18conv3x3_lds_kernelILi2ELi1ELi4ELb1ELi0ELi0ELi4ELi4ELi0ELb0EEEvNS_8ConvArgsEPKDF16_iiiiiiii", "conv3x3s2_lds_mt1_nt4"),
    ("_ZN4irmv18conv3x3_lds_kernelILi1ELi2ELi4ELb0ELi4ELi0ELi2ELi4ELi0ELb0EEEvNS_8ConvArgsEPKDF16_iiiiiiii", "conv3x3s1_lds_mt2_nt4+1x1"),
    ("_ZN4irmv18conv3x3_lds_kernelILi1ELi2ELi4ELb0ELi0ELi0ELi0ELi8ELi2ELb0EEEvNS_8ConvArgsEPKDF16_iiiiiiii", "conv3x3s1_wres"),
    ("_ZN4irmv18conv3x3_lds_kernelILi1ELi2ELi4ELb1ELi1ELi0ELi0ELi8ELi2ELb1EEEvNS_8ConvArgsEPKDF16_iiiiiiii", "conv3x3s1_wres_pp+1x1"),
    ("void irmv::conv3x3_lds_kernel<1, 4, 4, true, 0>(irmv::ConvArgs, __half const*, int, int, int, int)", "conv3x3s1_lds_mt4_nt4"),
    ("void irmv::conv_mfma_kernel<1, 1, 4, 2, false, 1, false, false, false>(irmv::ConvArgs)", "conv1x1s1_mt4_nt2"),
    ("void irmv::conv_mfma_kernel<3, 2, 1, 1, true, 1, false>(irmv::ConvArgs)", "conv3x3s2_mt1_nt1_c16"),
    ("void irmv::conv_mfma_kernel<1, 1, 1, 1, false, 0, true, false, false>(irmv::ConvArgs)", "conv1x1s1_mt1_nt1_f32"),
    ("void irmv::conv_mfma_kernel<3, 1, 1, 2, false, 1, false, true, true>(irmv::ConvArgs)", "conv3x3s1_mt1_nt2_deep_ct"),
    ("void irmv::c2f32_kernel<0, 6, false>(irmv::C2f32Args, int, int)", "c2f32_ab"),
    ("void irmv::c2f32_kernel<1, 2, true>(irmv::C2f32Args, int, int)", "c2f32_a"),
    ("void irmv::c2f32_kernel<2, 1, true>(irmv::C2f32Args, int, int)", "c2f32_b"),
    ("void irmv::kpt3_kernel<2>(irmv::Kpt3Args, int, int, int)", "kpt3_c128"),
    ("_ZN4irmv11kpt3_kernelILi4EEEvNS_8Kpt3ArgsEiii", "kpt3_c256"),
    ("void irmv::box_gather_kernel<1, true>(irmv::BoxGatherArgs, int)", "box_gather_c64"),
    ("_ZN4irmv17box_gather_kernelILi2ELb0EEEvNS_13BoxGatherArgsEi", "box_gather_c128"),
    ("irmv::cand_list_kernel(irmv::CandListArgs, int)", "cand_list"),
    ("void irmv::bneck64_kernel<1, 6, false>(irmv::BneckArgs)", "bneck64_b"),
    ("_ZN4irmv14bneck64_kernelILi0ELi6ELb1EEEvNS_9BneckArgsE", "bneck64_a"),
    ("void irmv::front_kernel<8>(irmv::FrontArgs, int, int)", "front_fused"),
    ("irmv::c2f2_kernel(irmv::C2fArgs, int, int)", "c2f2_fused"),
    ("void irmv::light_extract_kernel<false>(irmv::LightArgs)", "light_extract"),
    ("irmv::preprocess_kernel(irmv::PreArgs)", "preprocess"),
    ("irmv::conv0_kernel(irmv::Conv0Args)", "conv0_mfma"),
    ("irmv::sppf_pool_lds_kernel(__half*, int, int, int, int)", "sppf_pool"),
    ("irmv::scan_decode_kernel(irmv::PostArgs, int)", "decode"),
    ("void irmv::nms_pnp_kernel<false>(irmv::PostArgs)", "nms_pnp"),
    ("irmv::tile_merge_kernel(irmv::TileArgs, int)", "irmv::tile_merge_kernel(irmv::TileArgs, int)"),   # unknown to the table: the symbol itself
]


@pytest.mark.parametrize("sym,name", POINTWISE + OTHERS)
def test_symbol_maps_to_its_profile_name(sym, name):
    assert _names.internal_name(sym) == name
