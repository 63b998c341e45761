"""The variant matrix of the fused projection backward + Adam (csrc/gs_project.hip: `project_bwd_adam()`, the GS_PB / GS_PBC / GS_PBK
dispatch): one row per kernel family x regulariser mask, with the entry point of include/gs_raster.h that `TrainStepGraph(fuse_adam=True)`
reaches it through and the kernel the dispatch selects per SH degree D.  Plain data -- no torch, no library: shared by
tests/test_gpu_fused_variants.py (which runs every row at every degree) and tests/test_stage_calls_host.py (which holds the table to the
header: an entry point added later cannot arrive without a row here)."""
from collections import namedtuple

# tag: what a test prints; family: plain | poses | depth | ortho | fisheye | aa; scale / budget: the regulariser mask (the scale-ratio
# regulariser of LossComputer(lambda_scale=...), the budget regulariser of `mcmc=`); entry: the C ABI name; kernel: the instantiation
Variant = namedtuple("Variant", "tag family scale budget entry kernel")

MASKS = ((False, False), (True, False), (False, True), (True, True))   # none, scale, budget, scale + budget
_MASK_TAG = {(False, False): "", (True, False): "+scale", (False, True): "+budget", (True, True): "+scale+budget"}


def _plain(scale, budget):
    if budget:
        return "gs_project_bwd_adam_mcmc", f"project_bwd_budget_kernel<D, {3 if scale else 2}>"
    if scale:
        return "gs_project_bwd_adam_reg", "project_bwd_kernel<D, true, false, true>"
    return "gs_project_bwd_adam", "project_bwd_kernel<D, true, false>"


def _poses(scale, budget):
    if budget:
        return "gs_project_bwd_adam_sums", f"project_bwd_budget_kernel<D, {3 if scale else 2}, true>"
    return "gs_project_bwd_adam_sums", "project_bwd_kernel<D, true, true, true>" if scale else "project_bwd_kernel<D, true, true>"


def _depth(scale, budget):
    return "gs_project_bwd_adam_depth", f"project_bwd_depth_kernel<D, {4 + int(scale) + 2 * int(budget)}>"


def _camera(model):
    def row(scale, budget):
        assert not budget
        # (degree 4 with the regulariser under the fisheye: the branch-free kCamFisheyeSelect instantiation)
        return ("gs_project_bwd_adam_reg_cm" if scale else "gs_project_bwd_adam_cm",
                f"project_bwd_cm_kernel<D, true, {int(scale)}, {model}>")
    return row


def _aa(scale, budget):
    assert not budget
    return "gs_project_bwd_adam_reg_aa" if scale else "gs_project_bwd_adam_aa", f"project_bwd_aa_kernel<D, true, {int(scale)}>"


_FAMILIES = (("plain", _plain, MASKS), ("poses", _poses, MASKS), ("depth", _depth, MASKS), ("ortho", _camera("ortho"), MASKS[:2]),
             ("fisheye", _camera("fisheye"), MASKS[:2]), ("aa", _aa, MASKS[:2]))

VARIANTS = tuple(Variant(family + _MASK_TAG[mask], family, mask[0], mask[1], *row(*mask)) for family, row, masks in _FAMILIES for mask in masks)
BY_TAG = {v.tag: v for v in VARIANTS}
DEGREES = (0, 1, 2, 3, 4)
ENTRY_PREFIX = "gs_project_bwd_adam"
