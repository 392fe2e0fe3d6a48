"""The verbose build's check of the fused kernel's resources (mojosplat_amd/csrc/build.py, check_fused_kernel_resources)
reads the figures out of the compiler's remarks as the compiler writes them, and fires when one is exceeded."""
import pytest

from mojosplat_amd.csrc import build as hip_build

HALF = "_ZN12_GLOBAL__N_116k_sort_rasterizeILi3E6__halfLb1EEEvNS_10RasterArgsEN2ms9FusedSortE"
FLOAT = "_ZN12_GLOBAL__N_116k_sort_rasterizeILi3EfLb1EEEvNS_10RasterArgsEN2ms9FusedSortE"
OTHER = "_ZN12_GLOBAL__N_111k_tile_redoILi3EfEEvNS_10RasterArgsE"
TAIL = " [-Rpass-analysis=kernel-resource-usage]"


def _block(name, vgprs, scratch, lds, where="/src/csrc/rasterize.hip:784:1: remark: "):
    """One kernel's remarks, line for line as hipcc prints them (file:line:col first, then `remark:`)."""
    rows = [f"Function Name: {name}", "    TotalSGPRs: 104", f"    VGPRs: {vgprs}", "    AGPRs: 0",
            f"    ScratchSize [bytes/lane]: {scratch}", "    Dynamic Stack: False", "    Occupancy [waves/SIMD]: 6",
            "    SGPRs Spill: 0", "    VGPRs Spill: 0", f"    LDS Size [bytes/block]: {lds}"]
    return "".join(where + r + TAIL + "\n" for r in rows)


def test_figures_inside_the_limits_are_read_and_pass():
    got = hip_build.check_fused_kernel_resources(_block(OTHER, 138, 0, 44328) + _block(HALF, 80, 0, 46336) + _block(FLOAT, 80, 0, 46336))
    assert set(got) == {HALF, FLOAT}
    assert all(f == {"VGPRs": 80, "ScratchSize [bytes/lane]": 0, "LDS Size [bytes/block]": 46336} for f in got.values())
    # (the other layout clang has used: `remark:` first, then the position)
    hip_build.check_fused_kernel_resources(_block(HALF, 80, 0, 46336, "remark: rasterize.hip:682:0: ") +
                                           _block(FLOAT, 72, 0, 46336, "remark: rasterize.hip:682:0: "))


@pytest.mark.parametrize("vgprs,scratch,lds", [(81, 0, 46336), (80, 36, 46336), (80, 0, 46340)])
def test_a_figure_over_its_limit_fails_the_build(vgprs, scratch, lds):
    with pytest.raises(RuntimeError, match="over"):
        hip_build.check_fused_kernel_resources(_block(HALF, 80, 0, 46336) + _block(FLOAT, vgprs, scratch, lds))
    # another kernel's figures are not the fused kernel's
    hip_build.check_fused_kernel_resources(_block(HALF, 80, 0, 46336) + _block(FLOAT, 80, 0, 46336) + _block(OTHER, 138, 36, 50000))


def test_missing_figures_fail_the_build():
    with pytest.raises(RuntimeError, match="expected 2"):
        hip_build.check_fused_kernel_resources(_block(HALF, 80, 0, 46336))
    names_only = "".join(f"/src/rasterize.hip:784:1: remark: Function Name: {n}{TAIL}\n" for n in (HALF, FLOAT))
    with pytest.raises(RuntimeError, match="expected 2"):
        hip_build.check_fused_kernel_resources(names_only)
    with pytest.raises(RuntimeError, match="expected 2"):
        hip_build.check_fused_kernel_resources("")
