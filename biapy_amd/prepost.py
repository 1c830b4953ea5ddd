"""Input normalisation and output binarisation on the device.

Mirrors ``biapy/data/norm.py`` (``percentile_clip`` :395-473, ``zero_mean_unit_variance_normalization`` :586-645) and the
binarisation of ``biapy/engine/semantic_seg.py:418-431`` (``threshold_otsu`` of the merged prediction, then ``pred > th``)
for float32 tensors that already live on the MI355X - the 1024^3 volume of cfg 3 is 4.3 GB, and the reference takes its
percentiles / histogram on the host.

* percentiles are EXACT: the two order statistics ``np.percentile`` interpolates between come from a 4-pass radix select
  (``bpx_select_kth_f32``) and the interpolation repeats NumPy's float32 ``_lerp`` arithmetic, so the bounds are bit-identical;
* the histogram repeats ``np.histogram``'s float32 bin arithmetic (``bpx_histogram_f32``): identical counts, hence the
  identical Otsu threshold;
* mean / std use double accumulation on the device (NumPy: float32 pairwise sums) - equal to ~1e-7 relative, not bitwise;
* ``label`` / ``component_sizes`` / ``remove_small_objects`` carry on from the binarised mask: connected components with
  ``scipy.ndimage.label``'s numbering bit for bit (``csrc/label.hip``), so the mask no longer leaves the device to be labelled;
* ``LabelStitcher`` / ``label_blocks`` join the labels of the blocks of a regular grid into the labels of the whole volume (``csrc/stitch.hip``): a
  union-find over label ids fed by the block shells, ``scipy.ndimage.label``'s numbering bit for bit, so labelling is not bound to one call's 2^31 voxels;
* ``distance_transform_edt`` / ``label_distance`` give the exact Euclidean distance map of the mask or of the labels
  (``csrc/edt.hip``): on a unit grid ``scipy.ndimage.distance_transform_edt`` bit for bit;
* ``distance_transform_edt(return_indices=...)`` adds the nearest background voxel itself (``csrc/edt_index.hip``; among equally near ones the
  raster-first - product-defined, checked against a host twin), and ``expand_labels`` / ``voronoi_on_mask`` on top of it grow the instances by
  a distance without merging them and hand every masked voxel to its nearest instance;
* ``watershed`` floods an image from the seeds of ``label`` inside a mask (``csrc/watershed.hip``): the marker-controlled watershed those two
  lead up to, with exactly stated semantics of its own (ties go to the raster-first edge) - product-defined, checked against a host twin;
* ``label_overlap`` / ``matching`` judge the instances: the sparse contingency table of two label volumes (``csrc/overlap.hip``) and the
  reference's IoU matcher (tp / fp / fn, F1, panoptic quality) on top of it, with only the table's rows leaving the device;
* ``region_props`` / ``centroids`` / ``select_objects`` measure them: area, half-open bounding box, exact coordinate sums and centroid of every
  label (``csrc/regionprops.hip``; scikit-image's ``regionprops``, SciPy's ``find_objects`` / ``center_of_mass``, the integers bit for bit), and
  the filter that keeps the labels a torch expression over those tensors selects - the detection workflow's centroids and the instance
  workflow's property filter without a device-to-host copy of the label volume;
* ``shape_props`` and ``elongation`` / ``axis_lengths`` / ``surface_area`` / ``sphericity`` / ``perimeter`` / ``circularity`` finish that
  filter (``csrc/shapeprops.hip``): exact second-order coordinate sums, the covariance from their exact 128-bit numerator, voxel faces per axis
  and the weight classes of scikit-image's 2-D perimeter - integer sums, bit for bit a NumPy twin - and the measures as torch expressions;
* ``intensity_props`` measures an image over them (``csrc/intensityprops.hip``): minimum, maximum, the EXACT sum in ``int64`` limbs, that sum
  rounded once to ``float64`` (``math.fsum``'s value) and the mean of every label, for ``float32``, ``uint8`` and ``uint16`` images - the mean
  foreground probability of an instance as its confidence, one ``select_objects`` away;
* ``binary_erosion`` / ``binary_dilation`` / ``binary_opening`` / ``binary_closing``, ``erosion`` / ``dilation``, ``find_boundaries``,
  ``binary_fill_holes`` and ``clear_border`` are the steps between those calls (``csrc/morph.hip``: one 3 x 3 x 3 stencil pass over ``uint8``,
  ``int32`` or ``float32``; the structuring element is ``generate_binary_structure(ndim, connectivity)``): ``scipy.ndimage``'s ``binary_*``,
  ``grey_erosion`` / ``grey_dilation`` and ``binary_fill_holes`` bit for bit, Euclidean balls (``radius=``) through the exact distance
  transform, hole filling and border clearing through ``label`` / ``select_objects`` and the labels on the volume's faces;
* ``peak_local_max`` / ``peak_mask`` find the local maxima of a probability or distance map (``csrc/peaks.hip``): the detection workflow's
  points as a sorted, compact list that is never read back, and the markers of the "distance map -> peaks -> ``label`` -> ``watershed``"
  recipe as a 0 / 1 volume.  The call shape of ``skimage.feature.peak_local_max`` with a box of per-axis radii and semantics of its own (among
  equal values the raster-first voxel wins, so no two peaks lie in each other's box) - product-defined, checked against a host twin;
* ``median_filter`` / ``median_filter_axes`` smooth a probability map or a mask before any of that (``csrc/median.hip``): the first step of
  the reference's post-processing, ``scipy.ndimage.median_filter`` with a per-axis size as values and a NumPy twin bit for bit - exact
  selection on order-preserving keys in LDS and registers, ``float32`` / ``uint8`` / ``bool``, windows of up to 125 voxels;
* ``separable_filter`` / ``gaussian_filter`` / ``gaussian_laplace`` are the linear smoothing next to it (``csrc/sepfilter.hip``): one pass per
  axis with run-time weights of up to 65 taps, ``scipy.ndimage.correlate1d`` / ``gaussian_filter`` / ``gaussian_laplace`` in a stated
  ``float32`` arithmetic - a NumPy twin bit for bit, SciPy's ``float64`` result within a derived per-element bound.

Any contiguous float32 tensor is taken as it is, 16-byte aligned or not (``stack[1]`` of a batch with an odd element count per item is not):
the scans then read four 4-byte words where they would read one 16-byte word, and return the same bits.

NaN.  ``minmax`` returns ``(nan, nan)`` as soon as the data holds one NaN, as ``ndarray.min()`` / ``.max()`` do; ``histogram``, and with it
``threshold_otsu`` / ``binarize`` without a given threshold, then raise ``ValueError`` as ``np.histogram`` does for a range that is not
finite (an infinity in the data does the same), and such data never counts as binary.  ``mean_std`` and the normalisation carry the NaN
through, as NumPy.  ``kth_values`` / ``percentile`` / ``percentile_clip`` on data with NaN are UNSPECIFIED (NumPy returns NaN; the radix
select ranks a NaN by its bit pattern, beyond the infinities of its sign), and the class arg-max never lets a NaN win where ``np.argmax``
returns the first NaN (``csrc/prepost.hip``).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib as L

lib = L.lib


def _flat(x: torch.Tensor) -> torch.Tensor:
    if not x.is_cuda:
        raise RuntimeError("biapy_amd.prepost runs on the MI355X only (tensor is on %s); there is no CPU path" % x.device)
    if x.dtype != torch.float32:
        raise NotImplementedError(f"biapy_amd.prepost works on float32 tensors (got {x.dtype})")
    return x.contiguous().view(-1)


def kth_values(x: torch.Tensor, ranks) -> list:
    """Exact order statistics x_sorted[k] (0-based) for every k in ``ranks`` as Python floats (one host sync at the end)."""
    f = _flat(x)
    ws = torch.empty(int(lib.bpx_select_workspace()), dtype=torch.uint8, device=f.device)
    out = torch.empty(len(ranks), dtype=torch.float32, device=f.device)
    for q, k in enumerate(ranks):
        L.check(lib.bpx_select_kth_f32(f.data_ptr(), f.numel(), int(k), out.data_ptr() + 4 * q, ws.data_ptr(), L.stream_ptr()))
    return [float(v) for v in out.cpu().numpy()]


def percentile(x: torch.Tensor, q: float) -> float:
    """``float(np.percentile(x, q))`` (method 'linear') of a float32 tensor without sorting: two exact order statistics, then
    NumPy's arithmetic repeated operation by operation.  For a float32 array NumPy (>= 2) works in float32 throughout:
    ``quantile = q / float32(100)``, virtual index ``(n - 1) * quantile``, ``gamma = index - floor(index)`` and the ``_lerp``
    ``a + (b - a) * gamma`` (``b - (b - a) * (1 - gamma)`` for gamma >= 0.5) - numpy/lib/_function_base_impl.py."""
    return _percentile_of(x.numel(), q, lambda ranks: kth_values(x, ranks))


def _percentile_of(n: int, q: float, kth) -> float:
    """The host arithmetic of ``percentile`` on its own: ``kth(ranks)`` returns the order statistics at the two ranks asked for."""
    vi = np.float32(n - 1) * (np.float32(q) / np.float32(100))
    lo = int(math.floor(float(vi)))
    hi = min(lo + 1, n - 1)
    t = np.float32(vi - np.float32(lo))
    a, b = (np.float32(v) for v in kth([lo, hi]))
    d = np.float32(b - a)
    if t >= 0.5:
        return float(np.float32(b - np.float32(d * np.float32(np.float32(1) - t))))
    return float(np.float32(a + np.float32(d * t)))


def minmax(x: torch.Tensor) -> Tuple[float, float]:
    f = _flat(x)
    part = torch.empty((lib.bpx_scan_blocks(f.numel()), 2), dtype=torch.float32, device=f.device)
    L.check(lib.bpx_minmax_f32(f.data_ptr(), f.numel(), part.data_ptr(), L.stream_ptr()))
    return float(part[:, 0].min()), float(part[:, 1].max())


def _is_binary(x: torch.Tensor) -> bool:
    mn, mx = minmax(x)      # norm.py:38-42: a channel holding only 0 / 1 is never clipped or normalised
    return mn >= 0.0 and mx <= 1.0 and bool(((x == 0) | (x == 1)).all())


def percentile_clip(data: torch.Tensor, per_lower_bound: Optional[float] = None, per_upper_bound: Optional[float] = None,
                    lower_bound_val: Optional[float] = None, upper_bound_val: Optional[float] = None, apply_norm: bool = True):
    """Device counterpart of ``biapy.data.norm.percentile_clip`` on its NumPy branch (bounds from ``np.percentile``)."""
    if _is_binary(data):
        return data, 0.0, 1.0
    if per_lower_bound is None or per_lower_bound == -1:
        assert lower_bound_val is not None, "If 'per_lower_bound' is not provided, 'lower_bound_val' should be provided"
        x_lwr = lower_bound_val
    else:
        assert per_lower_bound > 0, "Value in 'per_lower_bound' should be less than 100"
        x_lwr = percentile(data, per_lower_bound)
    if per_upper_bound is None or per_upper_bound == -1:
        assert upper_bound_val is not None, "If 'per_upper_bound' is not provided, 'upper_bound_val' should be provided"
        x_upr = upper_bound_val
    else:
        assert per_upper_bound < 100, "Value in 'per_upper_bound' should be less than 100"
        x_upr = percentile(data, per_upper_bound)
    if apply_norm:
        out = torch.empty_like(data, memory_format=torch.contiguous_format)
        L.check(lib.bpx_clip_affine_f32(_flat(data).data_ptr(), data.numel(), x_lwr, x_upr, 0.0, 1.0, out.data_ptr(), L.stream_ptr()))
        data = out
    return data, x_lwr, x_upr


def mean_std(x: torch.Tensor) -> Tuple[float, float]:
    """Population mean / std (``ndarray.mean()`` / ``ndarray.std()``), two passes, double accumulation."""
    f = _flat(x)
    nb = lib.bpx_scan_blocks(f.numel())
    part = torch.empty(nb, dtype=torch.float64, device=f.device)
    L.check(lib.bpx_moment_f32(f.data_ptr(), f.numel(), 0.0, 1, part.data_ptr(), L.stream_ptr()))
    mean = float(part.sum()) / f.numel()
    L.check(lib.bpx_moment_f32(f.data_ptr(), f.numel(), mean, 2, part.data_ptr(), L.stream_ptr()))
    return mean, math.sqrt(float(part.sum()) / f.numel())


def zero_mean_unit_variance_normalization(data: torch.Tensor, mean: Optional[float] = None, std: Optional[float] = None,
                                          apply_norm: bool = True, eps: float = 1e-6):
    """Device counterpart of ``biapy.data.norm.zero_mean_unit_variance_normalization`` (NumPy branch)."""
    assert data.dim() >= 2, "Data should be at least 2D. E.g. (y, x) in 2D and (z, y, x) in 3D"
    if _is_binary(data):
        return data, 0.0, 1.0
    if mean is None or std is None:
        m, s = mean_std(data)
        mean = m if mean is None else mean
        std = s if std is None else std
    if apply_norm:
        out = torch.empty_like(data, memory_format=torch.contiguous_format)
        L.check(lib.bpx_clip_affine_f32(_flat(data).data_ptr(), data.numel(), -math.inf, math.inf, mean, max(std, eps), out.data_ptr(),
                                        L.stream_ptr()))
        data = out
    return data, float(mean), float(std)


def histogram(x: torch.Tensor, nbins: int = 256) -> Tuple[np.ndarray, np.ndarray]:
    """``np.histogram(x, bins=nbins, range=(x.min(), x.max()))`` of a float32 tensor: (counts int64, float32 edges)."""
    return _histogram(x, nbins, *minmax(x))


def _bin_edges(mn: float, mx: float, nbins: int) -> np.ndarray:
    """The float32 edge table ``np.histogram`` builds for ``range=(mn, mx)``, and its two refusals: a range that is not finite (a NaN or an
    infinity in the data) and edges that float32 cannot keep strictly increasing - counting into duplicate edges would be meaningless."""
    first, last = np.float32(mn), np.float32(mx)
    if not (np.isfinite(first) and np.isfinite(last)):
        raise ValueError(f"autodetected range of [{first}, {last}] is not finite")
    if first == last:                                    # numpy widens an empty range by +-0.5
        first, last = np.float32(first - np.float32(0.5)), np.float32(last + np.float32(0.5))
    edges = np.linspace(first, last, nbins + 1, endpoint=True, dtype=np.float32)
    if np.any(edges[:-1] >= edges[1:]):
        raise ValueError(f"Too many bins for data range. Cannot create {nbins} finite-sized bins.")
    return edges


def _histogram(x: torch.Tensor, nbins: int, mn: float, mx: float) -> Tuple[np.ndarray, np.ndarray]:
    f = _flat(x)
    edges = _bin_edges(mn, mx, nbins)                    # refuses before anything is launched
    first, last = edges[0], edges[-1]
    ed = torch.from_numpy(edges).to(f.device)
    counts = torch.zeros(nbins, dtype=torch.int64, device=f.device)
    L.check(lib.bpx_histogram_f32(f.data_ptr(), f.numel(), float(first), float(last), nbins, ed.data_ptr(), counts.data_ptr(), L.stream_ptr()))
    return counts.cpu().numpy(), edges


def threshold_otsu(x: torch.Tensor, nbins: int = 256) -> float:
    """skimage.filters.threshold_otsu on the device histogram (Otsu 1979: arg-max of the between-class variance over the
    bin centres).  The counts are bit-identical to np.histogram's, the few float64 operations below follow scikit-image."""
    mn, mx = minmax(x)
    if mn == mx:                                         # a constant volume (a blank tile): the value itself, so `x > th` is empty - as scikit-image
        return float(mn)
    counts, edges = _histogram(x, nbins, mn, mx)
    centers = (edges[:-1] + edges[1:]) / 2
    c = counts.astype(np.float64)
    w1, w2 = np.cumsum(c), np.cumsum(c[::-1])[::-1]
    m1 = np.cumsum(c * centers) / w1
    m2 = (np.cumsum((c * centers)[::-1]) / w2[::-1])[::-1]
    var12 = w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2
    return float(centers[int(np.argmax(var12))])


def binarize(pred: torch.Tensor, threshold: Optional[float] = None) -> torch.Tensor:
    """``(pred > threshold_otsu(pred)).astype(np.uint8)`` (semantic_seg.py:425-427) as a uint8 device tensor."""
    th = threshold_otsu(pred) if threshold is None else float(threshold)
    f = _flat(pred)
    out = torch.empty(pred.shape, dtype=torch.uint8, device=pred.device)
    L.check(lib.bpx_threshold_u8(f.data_ptr(), f.numel(), th, out.data_ptr(), L.stream_ptr()))
    return out


# ---- connected components of the binarised mask (csrc/label.hip) ----------------------------------------------------------------
# What follows binarize() in every segmentation workflow of the reference: label(seed_map) ahead of the instance watershed, the
# detection workflow's blobs, object counts and small-object removal of semantic masks (skimage.measure.label / scipy.ndimage.label
# on the host there).  The watershed is watershed() below, the matcher matching() at the end; the labels of several calls are joined by LabelStitcher / label_blocks, next section.

def _label_volume(t: torch.Tensor, what: str) -> Tuple[int, int, int]:
    if t.dim() not in (2, 3):
        raise ValueError(f"biapy_amd.prepost.{what} takes a 2-D (Y, X) or 3-D (Z, Y, X) tensor (got {t.dim()} dimensions)")
    if t.numel() >= 2 ** 31:
        raise NotImplementedError(f"biapy_amd.prepost.{what}: {t.numel()} voxels - volumes of 2^31 voxels or more are not supported (int32 indices)")
    return (1,) + tuple(t.shape) if t.dim() == 2 else tuple(t.shape)


def label(mask: torch.Tensor, connectivity: Optional[int] = None, return_num: bool = False):
    """``skimage.measure.label(mask, connectivity=connectivity, return_num=return_num)`` of a binary 2-D / 3-D ``uint8`` or ``bool`` device
    tensor: an ``int32`` tensor of the same shape, 0 for background, the components numbered ``1..N`` in raster order of each component's
    first voxel - bit for bit ``scipy.ndimage.label(mask, generate_binary_structure(mask.ndim, connectivity))``.  ``connectivity`` 1 joins
    faces, 2 faces and edges, 3 (3-D only) corners too; ``None`` is the full connectivity ``mask.ndim``.

    Two differences from scikit-image, both on purpose: with ``return_num`` the count comes back as a 0-d ``int32`` DEVICE tensor, so the
    call never waits for the device (it is a fixed sequence of six launches and can be captured in a graph); and the input is binary - every
    nonzero value is foreground, regions of different nonzero values are NOT separated.  Other dtypes raise ``NotImplementedError``, as does
    a volume of 2^31 voxels or more (before anything is launched); a CPU tensor raises ``RuntimeError``: there is no CPU path."""
    if mask.dtype not in (torch.uint8, torch.bool):
        raise NotImplementedError(f"biapy_amd.prepost.label works on uint8 or bool masks (got {mask.dtype}); binarize() makes one")
    if not mask.is_cuda:
        raise RuntimeError("biapy_amd.prepost runs on the MI355X only (tensor is on %s); there is no CPU path" % mask.device)
    Z, Y, X = _label_volume(mask, "label")
    c = mask.dim() if connectivity is None else int(connectivity)
    if not 1 <= c <= mask.dim():
        raise ValueError(f"connectivity must be in 1..{mask.dim()} for a {mask.dim()}-D mask (got {connectivity})")
    m = mask.contiguous()
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    need = int(lib.bpx_label_workspace(Z, Y, X))
    if need < 0:
        raise NotImplementedError(f"biapy_amd.prepost.label: a {tuple(mask.shape)} volume is refused (an empty axis, or 2^31 voxels or more)")
    ws = torch.empty(need, dtype=torch.uint8, device=m.device)
    out = torch.empty(mask.shape, dtype=torch.int32, device=m.device)
    num = torch.empty((), dtype=torch.int32, device=m.device)
    L.check(lib.bpx_label_u8(m.data_ptr(), Z, Y, X, c, out.data_ptr(), num.data_ptr(), ws.data_ptr(), need, L.stream_ptr()))
    return (out, num) if return_num else out


def _labels(labels: torch.Tensor, what: str) -> torch.Tensor:
    if labels.dtype != torch.int32:
        raise NotImplementedError(f"biapy_amd.prepost.{what} works on the int32 labels of label() (got {labels.dtype})")
    if not labels.is_cuda:
        raise RuntimeError("biapy_amd.prepost runs on the MI355X only (tensor is on %s); there is no CPU path" % labels.device)
    if labels.numel() < 1 or labels.numel() >= 2 ** 31:
        raise NotImplementedError(f"biapy_amd.prepost.{what}: {labels.numel()} voxels - empty volumes and volumes of 2^31 voxels or more are not supported")
    return labels


def component_sizes(labels: torch.Tensor, num) -> torch.Tensor:
    """``np.bincount(labels.ravel(), minlength=num + 1)[:num + 1]`` as an ``int32`` device tensor: entry 0 counts the background, entry ``l``
    the voxels of component ``l``; labels above ``num`` are not counted.  ``num``: a Python int (no wait for the device; inside a graph an
    upper bound of the count serves, the entries past ``N`` are 0), or the 0-d tensor ``label(..., return_num=True)`` returns, which is read
    back here."""
    lab = _labels(labels, "component_sizes").contiguous()
    n_max = int(num)
    if n_max < 0:
        raise ValueError(f"num must not be negative (got {n_max})")
    sizes = torch.empty(n_max + 1, dtype=torch.int32, device=lab.device)
    L.check(lib.bpx_label_sizes(lab.data_ptr(), lab.numel(), n_max, sizes.data_ptr(), L.stream_ptr()))
    return sizes


def remove_small_objects(labels: torch.Tensor, min_size: int = 64, relabel: bool = False, num=None, return_num: bool = False):
    """``skimage.morphology.remove_small_objects(labels, min_size)`` on an ``int32`` label image: a NEW tensor in which every component
    with fewer than ``min_size`` voxels is 0.  The survivors keep their ids, as in scikit-image; ``relabel=True`` renumbers them ``1..N'`` in
    the same order.  ``num``: the largest label (an int, or the device count of ``label``); ``None`` reads ``labels.max()`` back.
    ``return_num`` adds ``N'``, the number of survivors, as a 0-d ``int32`` device tensor."""
    lab = _labels(labels, "remove_small_objects")
    n_max = int(lab.max()) if num is None else int(num)
    sizes = component_sizes(lab, n_max)
    out = lab.clone(memory_format=torch.contiguous_format)
    left = torch.empty((), dtype=torch.int32, device=lab.device)
    L.check(lib.bpx_label_filter(out.data_ptr(), out.numel(), n_max, sizes.data_ptr(), int(min_size), 1 if relabel else 0, left.data_ptr(),
                                 L.stream_ptr()))
    return (out, left) if return_num else out


# ---- labels of several calls joined into the labels of the whole volume (csrc/stitch.hip, csrc/stitch_core.h) ----------------------------------
# Every call above and below ends at 2^31 voxels, and watershed()'s workspace makes per-block processing the only route for large volumes long
# before that; the predictors of chunked.py deliver volumes of any size.  LabelStitcher joins what the calls on the blocks of a regular grid
# produce - a union-find over label ids, fed by the voxels on the block shells alone, and one renumbering pass - and label_blocks is label() for
# a mask of any size on top of it.  Not offered: overlapping blocks (halo matching by IoU), blocks resident on the host or on other GPUs (only
# the shells would have to travel: the named follow-up), any other call past 2^31 voxels, int64 labels, more than 3 dimensions.

def _grid_shapes(shape, block_shape, what: str):
    shape = tuple(int(v) for v in shape)
    if len(shape) not in (2, 3):
        raise ValueError(f"biapy_amd.prepost.{what} takes a 2-D (Y, X) or 3-D (Z, Y, X) shape (got {len(shape)} dimensions)")
    if min(shape) < 1:
        raise ValueError(f"biapy_amd.prepost.{what}: every extent must be at least 1 (got {shape})")
    block = tuple(int(v) for v in block_shape)
    if len(block) != len(shape):
        raise ValueError(f"biapy_amd.prepost.{what}: block_shape must have {len(shape)} entries for a {len(shape)}-D shape (got {block})")
    if min(block) < 1:
        raise ValueError(f"biapy_amd.prepost.{what}: block extents must be at least 1 (got {block})")
    block = tuple(min(b, s) for b, s in zip(block, shape))
    if math.prod(block) >= 2 ** 31:
        raise NotImplementedError(f"biapy_amd.prepost.{what}: {math.prod(block)} voxels per block - blocks of 2^31 voxels or more are not supported (int32 indices)")
    if len(shape) == 2:
        shape, block = (1,) + shape, (1,) + block
    return shape, block


class LabelStitcher:
    """Joins the ``int32`` labels of the blocks of a regular grid into the labels of the whole volume, in place and on the device.

    The volume ``shape`` (2-D is handled as ``Z = 1``) is cut every ``block_shape``; the last block of an axis may be ragged; block ``(i, j, k)``
    covers ``[i*bz, min((i+1)*bz, Z))`` and likewise in y and x.  Each block is a contiguous ``int32`` device tensor of its own with local labels
    ``1..n_b`` (``<= 0`` or ``> n_b``: background) - what ``label`` or ``watershed`` returns for it.  Two uniting rules:

    * ``rule="touch"`` (connected components): two labels are united when a voxel of one has a voxel of the other among its neighbours at
      ``connectivity`` in ANOTHER block - across faces, and at connectivity 2 and 3 across block edges and corners too.  On blocks that ``label``
      produced at the same connectivity the result is ``scipy.ndimage.label`` of the whole mask BIT FOR BIT.
    * ``rule="contact"`` (instances, e.g. per-block ``watershed``; connectivity 1 only; product-defined, checked against a host twin,
      ``tests/stitch_ref.py``): only face-adjacent blocks take part.  For A (low side) and B (high side) along an axis, ``c(a, b)`` counts the
      in-plane positions where A's last plane holds ``a`` and B's first plane holds ``b``, ``s_A(a)`` / ``s_B(b)`` the positions of each plane that
      hold the label, partner or not; ``a`` and ``b`` are united iff ``c(a, b) * q >= p * min(s_A(a), s_B(b))`` with ``min_contact = (p, q)``
      integers, ``0 < p <= q <= 32768``.  UNIONS ARE TRANSITIVE: a chain of contacts fuses into one object, whatever the ratio between its ends.

    Numbering: the merged objects are ``1..M`` in raster order of each object's first voxel in the WHOLE volume - ``scipy.ndimage.label``'s.

    ``add(index, labels, num)`` registers a block, ``resolve()`` returns ``M`` as a 0-d ``int32`` device tensor (``-1``: more than ``max_labels``
    labels over all blocks, or at ``"contact"`` more distinct pairs on the faces than the table holds), ``apply()`` renumbers all blocks in place
    (on overflow they stay as they were).  ``max_labels`` defaults to ``min(total voxels, 2**22)`` and sizes five tables of 4 to 8 bytes per entry.
    ``resolve()`` + ``apply()`` are a launch sequence fixed by the grid, read nothing back and can be captured in a graph and replayed on
    overwritten block contents; ``add`` uploads a descriptor and is NOT capturable.  No float arithmetic: the same bits every run."""

    def __init__(self, shape, block_shape, connectivity: int = 1, rule: str = "touch", min_contact=(1, 2), max_labels: Optional[int] = None):
        self.ndim = len(tuple(shape))
        self.shape, self.block_shape = _grid_shapes(shape, block_shape, "LabelStitcher")
        c = int(connectivity)
        if not 1 <= c <= self.ndim:
            raise ValueError(f"connectivity must be in 1..{self.ndim} for a {self.ndim}-D volume (got {connectivity})")
        if rule not in ("touch", "contact"):
            raise ValueError(f"rule must be 'touch' or 'contact' (got {rule!r})")
        if rule == "contact" and c != 1:
            raise ValueError(f"rule='contact' looks at block faces only: connectivity must be 1 (got {connectivity})")
        p, q = (int(v) for v in min_contact)
        if not 0 < p <= q <= 32768:
            raise ValueError(f"min_contact = (p, q) needs integers with 0 < p <= q <= 32768 (got {tuple(min_contact)})")
        total = math.prod(self.shape)
        t_max = min(total, 2 ** 22) if max_labels is None else int(max_labels)
        if not 1 <= t_max < 2 ** 31 - 1:
            raise ValueError(f"max_labels must be in [1, 2^31 - 1) (got {max_labels})")
        self.connectivity, self.rule, self.min_contact, self.max_labels = c, rule, (p, q), t_max
        self.grid = tuple(-(-s // b) for s, b in zip(self.shape, self.block_shape))
        self.nblocks = math.prod(self.grid)
        if self.nblocks >= 2 ** 20:
            raise NotImplementedError(f"biapy_amd.prepost.LabelStitcher: {self.nblocks} blocks - grids of 2^20 blocks or more are not supported")
        self._blocks = [None] * self.nblocks          # (labels, num: int / 0-d tensor / None)
        self._dev = None

    def _index(self, index) -> Tuple[int, int, int]:
        idx = tuple(int(v) for v in index)
        if len(idx) != self.ndim:
            raise ValueError(f"biapy_amd.prepost.LabelStitcher.add: index must have {self.ndim} entries (got {idx})")
        idx = (0,) * (3 - self.ndim) + idx
        if not all(0 <= v < g for v, g in zip(idx, self.grid)):
            raise ValueError(f"biapy_amd.prepost.LabelStitcher.add: block {idx[3 - self.ndim:]} lies outside the grid {self.grid[3 - self.ndim:]}")
        return idx

    def _extents(self, idx):
        origin = tuple(i * b for i, b in zip(idx, self.block_shape))
        return origin, tuple(min(o + b, s) - o for o, b, s in zip(origin, self.block_shape, self.shape))

    def _allocate(self, device) -> None:
        t = self.max_labels + 1
        self._dev = device
        self._nums = torch.zeros(self.nblocks, dtype=torch.int32, device=device)
        self._offs = torch.zeros(self.nblocks + 1, dtype=torch.int64, device=device)
        self._desc = torch.zeros((self.nblocks, 32), dtype=torch.uint8, device=device)
        self._parent = torch.empty(t, dtype=torch.int32, device=device)
        self._first = torch.empty(t, dtype=torch.int64, device=device)
        self._key = torch.empty(t, dtype=torch.int64, device=device)
        self._map = torch.zeros(t, dtype=torch.int32, device=device)
        self._flag = torch.ones((), dtype=torch.int32, device=device)      # up until the first resolve(): apply() before it writes nothing
        self._M = torch.full((), -1, dtype=torch.int32, device=device)
        self._iota = torch.arange(t, dtype=torch.int64, device=device)
        self._ws = None
        if self.rule == "contact":
            Z, Y, X = self.shape
            faces = (self.grid[0] - 1) * Y * X + (self.grid[1] - 1) * Z * X + (self.grid[2] - 1) * Z * Y
            self._max_pairs = max(1, min(faces, 2 ** 21))
            need = int(lib.bpx_stitch_contact_workspace(*self.shape, *self.block_shape, self.max_labels, self._max_pairs))
            if need < 0:
                raise NotImplementedError("biapy_amd.prepost.LabelStitcher: the block faces of this grid hold 2^31 positions or more")
            self._ws = torch.empty(max(need, 16), dtype=torch.uint8, device=device)

    def add(self, index, labels: torch.Tensor, num=None) -> None:
        """Registers block ``index`` (``(i, j, k)``; ``(j, k)`` in 2-D): an ``int32`` contiguous device tensor of exactly that block's extents,
        kept alive by the stitcher and renumbered in place by ``apply()``.  ``num``: the block's label count ``n_b`` as an int, or the 0-d device
        count of ``label(..., return_num=True)`` (read again, on the device, by every ``resolve()``); ``None`` takes ``labels.amax()`` on the
        device at every ``resolve()``.  Nothing is read back.  Uploads the block's descriptor: NOT capturable."""
        if labels.dtype != torch.int32:
            raise NotImplementedError(f"biapy_amd.prepost.LabelStitcher.add works on the int32 labels of label() / watershed() (got {labels.dtype})")
        if not labels.is_cuda:
            raise RuntimeError("biapy_amd.prepost runs on the MI355X only (tensor is on %s); there is no CPU path" % labels.device)
        idx = self._index(index)
        origin, ext = self._extents(idx)
        if labels.dim() != self.ndim or tuple(labels.shape) != ext[3 - self.ndim:]:
            raise ValueError(f"biapy_amd.prepost.LabelStitcher.add: block {idx[3 - self.ndim:]} has extents {ext[3 - self.ndim:]} (got a tensor of shape {tuple(labels.shape)})")
        if not labels.is_contiguous():
            raise ValueError("biapy_amd.prepost.LabelStitcher.add: the block must be contiguous (it is renumbered in place)")
        if isinstance(num, torch.Tensor):
            if num.dtype != torch.int32 or num.dim() != 0 or not num.is_cuda:
                raise ValueError(f"num must be an int or the 0-d int32 device count of label() (got a {num.dtype} tensor of shape {tuple(num.shape)} on {num.device})")
        elif num is not None:
            num = int(num)
            if not 0 <= num < 2 ** 31 - 1:
                raise ValueError(f"num must be in [0, 2^31 - 1) (got {num})")
        if self._dev is None:
            self._allocate(labels.device)
        elif labels.device != self._dev:
            raise ValueError(f"biapy_amd.prepost.LabelStitcher.add: the blocks must live on one device (got {labels.device} after {self._dev})")
        b = (idx[0] * self.grid[1] + idx[1]) * self.grid[2] + idx[2]
        d = L.StitchBlock(labels.data_ptr(), *origin, *ext)
        self._desc[b].copy_(torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8))
        if isinstance(num, int):
            self._nums[b] = num
        self._blocks[b] = (labels, num, origin, ext)

    def resolve(self) -> torch.Tensor:
        """Unites the labels across the blocks and numbers the merged objects: ``M`` as a 0-d ``int32`` device tensor (the same tensor at every
        call, so a graph replay refreshes it), ``-1`` on overflow.  Every block must have been added."""
        missing = [b for b, e in enumerate(self._blocks) if e is None]
        if missing:
            names = [tuple(np.unravel_index(b, self.grid))[3 - self.ndim:] for b in missing[:4]]
            raise ValueError(f"biapy_amd.prepost.LabelStitcher.resolve: {len(missing)} of {self.nblocks} blocks have not been added (first: "
                             + ", ".join(str(tuple(int(v) for v in n)) for n in names) + ")")
        s, t = L.stream_ptr(), self.max_labels
        Z, Y, X = self.shape
        for b, (lab, num, _, _) in enumerate(self._blocks):
            if num is None:
                torch.amax(lab.view(-1), dim=0, out=self._nums[b])
            elif isinstance(num, torch.Tensor):
                self._nums[b].copy_(num)
        L.check(lib.bpx_stitch_begin(self._nums.data_ptr(), self.nblocks, t, self._offs.data_ptr(), self._parent.data_ptr(), self._first.data_ptr(),
                                     self._key.data_ptr(), self._flag.data_ptr(), s))
        for b, (lab, _, origin, ext) in enumerate(self._blocks):
            L.check(lib.bpx_stitch_first(lab.data_ptr(), *ext, *origin, Y, X, self._nums.data_ptr() + 4 * b, self._offs.data_ptr() + 8 * b, t,
                                         self._first.data_ptr(), s))
        if self.rule == "touch":
            L.check(lib.bpx_stitch_shell(self._desc.data_ptr(), Z, Y, X, *self.block_shape, self.connectivity, self._nums.data_ptr(),
                                         self._offs.data_ptr(), t, self._parent.data_ptr(), s))
        else:
            L.check(lib.bpx_stitch_contact(self._desc.data_ptr(), Z, Y, X, *self.block_shape, self._nums.data_ptr(), self._offs.data_ptr(), t,
                                           *self.min_contact, self._max_pairs, self._parent.data_ptr(), self._flag.data_ptr(), self._ws.data_ptr(),
                                           self._ws.numel(), s))
        L.check(lib.bpx_stitch_resolve(self._parent.data_ptr(), self._first.data_ptr(), self._key.data_ptr(), self._offs.data_ptr() + 8 * self.nblocks,
                                       t, self._flag.data_ptr(), s))
        # the roots that hold a voxel, ranked by key: one sort over the fixed-size key table, as label_overlap ranks its pairs
        order = torch.sort(self._key).indices
        rank = torch.empty_like(order).scatter_(0, order, self._iota)
        live = self._key != torch.iinfo(torch.int64).max
        of_root = torch.where(live, rank + 1, 0).to(torch.int32)
        torch.index_select(of_root, 0, self._parent.to(torch.int64), out=self._map)
        self._M.copy_(torch.where(self._flag > 0, -1, live.sum()).to(torch.int32))
        return self._M

    def apply(self) -> None:
        """Renumbers every block in place with the map of the last ``resolve()``; background (``<= 0`` or ``> n_b``) becomes 0.  After an
        overflow - and before the first ``resolve()`` - nothing is written."""
        if self._dev is None or any(e is None for e in self._blocks):
            raise ValueError("biapy_amd.prepost.LabelStitcher.apply: resolve() comes first, after every block has been added")
        s = L.stream_ptr()
        for b, (lab, _, _, _) in enumerate(self._blocks):
            L.check(lib.bpx_stitch_apply(lab.data_ptr(), lab.numel(), self._nums.data_ptr() + 4 * b, self._offs.data_ptr() + 8 * b, self.max_labels,
                                         self._map.data_ptr(), self._flag.data_ptr(), s))


def label_blocks(mask: torch.Tensor, block_shape=None, connectivity: Optional[int] = None, return_num: bool = False, max_labels: Optional[int] = None):
    """``label`` for a binary 2-D / 3-D ``uint8`` or ``bool`` device mask of ANY size: the whole ``int32`` volume, numbered as ``label`` numbers it
    - ``scipy.ndimage.label`` bit for bit - by labelling block after block and stitching (``LabelStitcher``, rule ``"touch"``).

    ``block_shape=None`` takes the thickest Z slabs that stay below 2^31 voxels; a single slab means exactly ``label``'s launches.  Blocks
    ``(bz, Y, X)`` - Z slabs - are labelled and renumbered in place in contiguous views of the result, with no copies; any other block shape is
    copied in and out with torch.  With ``return_num`` the count comes back as a 0-d ``int32`` device tensor, ``-1`` when the blocks hold more than
    ``max_labels`` labels in all (default ``min(voxels, 2**22)``; the result is then the blocks' own numbering).

    Refused before anything is launched: other dtypes (``NotImplementedError``), a CPU tensor (``RuntimeError``), other ranks, block extents
    below 1 and a connectivity outside ``1..ndim`` (``ValueError``), a block or - without ``block_shape`` - one plane ``Y * X`` of 2^31 voxels or
    more (``NotImplementedError``)."""
    if mask.dtype not in (torch.uint8, torch.bool):
        raise NotImplementedError(f"biapy_amd.prepost.label_blocks works on uint8 or bool masks (got {mask.dtype}); binarize() makes one")
    if not mask.is_cuda:
        raise RuntimeError("biapy_amd.prepost runs on the MI355X only (tensor is on %s); there is no CPU path" % mask.device)
    if mask.dim() not in (2, 3):
        raise ValueError(f"biapy_amd.prepost.label_blocks takes a 2-D (Y, X) or 3-D (Z, Y, X) tensor (got {mask.dim()} dimensions)")
    nd = mask.dim()
    if block_shape is None:
        plane = math.prod(mask.shape[-2:])
        if plane >= 2 ** 31:
            raise NotImplementedError(f"biapy_amd.prepost.label_blocks: one plane Y * X has {plane} voxels - Z slabs of 2^31 voxels or more are not supported; give a block_shape")
        block_shape = tuple(mask.shape) if nd == 2 else (max(1, min(mask.shape[0], (2 ** 31 - 1) // max(plane, 1))),) + tuple(mask.shape[1:])
    shape, block = _grid_shapes(mask.shape, block_shape, "label_blocks")
    c = nd if connectivity is None else int(connectivity)
    if not 1 <= c <= nd:
        raise ValueError(f"connectivity must be in 1..{nd} for a {nd}-D mask (got {connectivity})")
    if block == shape:
        return label(mask, c, return_num)
    st = LabelStitcher(mask.shape, block[3 - nd:], c, "touch", max_labels=max_labels)
    m = mask.contiguous()
    m = (m.view(torch.uint8) if m.dtype == torch.bool else m).view(shape)
    out = torch.empty(shape, dtype=torch.int32, device=m.device)
    nums = torch.empty(st.nblocks, dtype=torch.int32, device=m.device)
    slabs = block[1:] == shape[1:]
    need = int(lib.bpx_label_workspace(*block))
    ws = torch.empty(need, dtype=torch.uint8, device=m.device)
    pieces = []
    for b in range(st.nblocks):
        idx = tuple(int(v) for v in np.unravel_index(b, st.grid))
        (z0, y0, x0), (ez, ey, ex) = st._extents(idx)
        src = m[z0:z0 + ez, y0:y0 + ey, x0:x0 + ex]
        if slabs:
            dst = out[z0:z0 + ez]
        else:
            src, dst = src.contiguous(), torch.empty((ez, ey, ex), dtype=torch.int32, device=m.device)
            pieces.append((dst, (z0, y0, x0)))
        L.check(lib.bpx_label_u8(src.data_ptr(), ez, ey, ex, c, dst.data_ptr(), nums.data_ptr() + 4 * b, ws.data_ptr(), need, L.stream_ptr()))
        st.add(idx[3 - nd:], dst if nd == 3 else dst.view(ey, ex), nums[b])
    num = st.resolve()
    st.apply()
    for dst, (z0, y0, x0) in pieces:
        out[z0:z0 + dst.shape[0], y0:y0 + dst.shape[1], x0:x0 + dst.shape[2]] = dst
    out = out.view(mask.shape)
    return (out, num) if return_num else out


# ---- exact Euclidean distance transform of the mask or of the labels (csrc/edt.hip, csrc/edt_index.hip) -----------------------------------
# What the instance workflow of the reference starts from after label(): the distance ("D") channel of its targets and the seeds of the
# marker-controlled watershed (scipy.ndimage.distance_transform_edt / the edt package on the host there), and - with the nearest background
# voxel beside the distance - skimage.segmentation.expand_labels and the reference's "Voronoi on mask" step.  Not offered: indices for
# label_distance, SciPy's choice among equally near voxels (the raster-first one is returned), a black border, more than 3 dimensions, 2^31
# voxels or more and multi-GPU slabs.  The D channel's normalisation is instance_targets() below (biapy_amd.targets); the watershed is watershed().

def _edt(t: torch.Tensor, what: str, label_mode: bool, sampling, squared: bool, distances: bool = True, indices: bool = False, invert: bool = False):
    """The distances (``indices=False``: through ``bpx_edt``, as ever), or ``(distances or None, linear indices)`` through ``bpx_edt_index``."""
    if t.dim() not in (2, 3):
        raise ValueError(f"biapy_amd.prepost.{what} takes a 2-D (Y, X) or 3-D (Z, Y, X) tensor (got {t.dim()} dimensions)")
    samp = None
    if sampling is not None:
        try:
            vals = [float(v) for v in sampling]
        except (TypeError, ValueError):
            vals = []
        if len(vals) != t.dim() or not all(math.isfinite(v) and v > 0.0 for v in vals):
            raise ValueError(f"biapy_amd.prepost.{what}: sampling must be {t.dim()} positive finite numbers, one per axis (got {sampling!r})")
        samp = (C.c_double * 3)(*([1.0] * (3 - len(vals)) + vals))
    if not t.is_cuda:
        raise RuntimeError("biapy_amd.prepost runs on the MI355X only (tensor is on %s); there is no CPU path" % t.device)
    Z, Y, X = _label_volume(t, what)
    if t.numel() < 1:
        raise NotImplementedError(f"biapy_amd.prepost.{what}: a {tuple(t.shape)} volume has an empty axis")
    need = int((lib.bpx_edt_index_workspace if indices else lib.bpx_edt_workspace)(Z, Y, X, 0 if samp is None else 1))
    if need < 0:
        raise NotImplementedError(f"biapy_amd.prepost.{what}: a {tuple(t.shape)} volume is refused on the exact integer path - Z^2 + Y^2 + X^2 must "
                                  "stay below 2^31 - 1 (the squared distance would reach the sentinel)")
    k = t.contiguous()
    if k.dtype == torch.bool:
        k = k.view(torch.uint8)
    dtype = L.I32 if k.dtype == torch.int32 else L.U8
    if indices and not distances and samp is None:
        need += 4 * t.numel()                                         # the integer path keeps its values in the distances: without them, in the workspace
    ws = torch.empty(need, dtype=torch.uint8, device=k.device)
    out = torch.empty(t.shape, dtype=torch.int32 if (squared and samp is None) else torch.float32, device=k.device) if distances else None
    if not indices:
        L.check(lib.bpx_edt(k.data_ptr(), dtype, 1 if label_mode else 0, Z, Y, X, samp, 1 if squared else 0, out.data_ptr(), ws.data_ptr(), need,
                            L.stream_ptr()))
        return out
    idx = torch.empty(t.shape, dtype=torch.int32, device=k.device)
    L.check(lib.bpx_edt_index(k.data_ptr(), dtype, 1 if invert else 0, Z, Y, X, samp, 1 if squared else 0, out.data_ptr() if distances else None,
                              idx.data_ptr(), ws.data_ptr(), need, L.stream_ptr()))
    return out, idx


def _unravel(idx: torch.Tensor) -> torch.Tensor:
    """(ndim, *shape) int32 coordinates of a linear-index volume; -1 stays -1 on every axis."""
    coords, rest = [], idx
    for n in reversed(idx.shape):
        coords.append(torch.where(idx < 0, idx, rest % n))
        rest = torch.div(rest, n, rounding_mode="floor")
    return torch.stack(coords[::-1])


def distance_transform_edt(mask: torch.Tensor, sampling=None, squared: bool = False, return_distances: bool = True, return_indices=False):
    """``scipy.ndimage.distance_transform_edt(mask, sampling=sampling)`` of a binary 2-D / 3-D ``uint8`` or ``bool`` device tensor: for every
    nonzero voxel the Euclidean distance to the nearest zero voxel, 0 on the zero voxels.  As in SciPy the volume border is no source.

    ``sampling=None`` is the exact path: the squared distance on a unit grid is an integer, computed as one.  ``squared=True`` returns it as
    ``int32``; otherwise the result is ``float32(sqrt(float64(squared)))`` - SciPy's float64 result rounded to ``float32``, bit for bit.  With
    ``sampling=(sz, sy, sx)`` (``(sy, sx)`` in 2-D; positive finite floats, anything else raises ``ValueError``) the work is done in fp64 and
    the result is the ``float32`` distance, or its square; a given ``sampling`` always takes that path, ``(1, 1, 1)`` too.

    ``return_indices`` adds WHICH zero voxel is the nearest (``csrc/edt_index.hip``).  ``"linear"`` returns an ``int32`` tensor of the mask's
    shape holding that voxel's linear index (C order), which is a third of the memory and what ``expand_labels`` / ``voronoi_on_mask`` use;
    ``True`` returns SciPy's form, an ``int32`` tensor of shape ``(ndim, *mask.shape)`` holding its coordinates.  With both results asked for
    the order is SciPy's, ``(distances, indices)``; ``return_distances=False`` returns the indices alone, and without indices raises
    ``ValueError``.  The distances beside indices are those of the plain call, bit for bit.  THE RULE for the index: among equally near zero
    voxels the one with the smallest linear index - the raster-first ``(z, y, x)`` - is returned; a zero voxel's index is its own.  SciPy
    breaks such ties another way, so on the exact path the returned voxel is at SciPy's distance but need not be SciPy's voxel.  With
    ``sampling`` the returned voxel is a nearest zero up to the fp64 path's rounding; which of several zeros whose fp64 costs differ only by
    rounding is returned is UNSPECIFIED.

    ONE DIFFERENCE from SciPy: a mask without any zero voxel has no nearest zero, and every voxel gets a sentinel - ``INT32_MAX`` in the
    ``int32`` result, ``+inf`` in the ``float32`` ones, ``-1`` in the indices (every coordinate) - where SciPy returns distances to a
    fictitious point.

    Three launches fixed by the shape and the path, nothing read back, the same bits every run: the call can be captured in a graph.
    Refused before anything is launched: a CPU tensor (``RuntimeError``); other dtypes, an empty axis, 2^31 voxels or more and, on the exact
    path, ``Z^2 + Y^2 + X^2 >= 2^31 - 1`` (``NotImplementedError``); other ranks (``ValueError``)."""
    if mask.dtype not in (torch.uint8, torch.bool):
        raise NotImplementedError(f"biapy_amd.prepost.distance_transform_edt works on uint8 or bool masks (got {mask.dtype}); binarize() makes "
                                  "one, label_distance() takes int32 labels")
    linear = isinstance(return_indices, str) and return_indices == "linear"
    if not linear and not isinstance(return_indices, (bool, np.bool_)):
        raise ValueError(f'biapy_amd.prepost.distance_transform_edt: return_indices must be False, True or "linear" (got {return_indices!r})')
    if not return_indices and not return_distances:
        raise ValueError("biapy_amd.prepost.distance_transform_edt: at least one of return_distances / return_indices must be asked for")
    if not return_indices:
        return _edt(mask, "distance_transform_edt", False, sampling, squared)
    dist, idx = _edt(mask, "distance_transform_edt", False, sampling, squared, distances=bool(return_distances), indices=True)
    if not linear:
        idx = _unravel(idx)
    return (dist, idx) if return_distances else idx


def _nearest_label(labels: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """labels at the linear indices ``idx`` (-1: a volume without any label, whose voxel 0 is background too)."""
    return torch.index_select(labels.contiguous().view(-1), 0, idx.clamp_min(0).view(-1)).view(labels.shape)


def expand_labels(labels: torch.Tensor, distance=1, sampling=None) -> torch.Tensor:
    """``skimage.segmentation.expand_labels(labels, distance=distance, spacing=sampling)`` of a 2-D / 3-D ``int32`` label tensor: a NEW ``int32``
    tensor in which every background voxel whose nearest labelled voxel is no farther than ``distance`` takes that voxel's label; labelled
    voxels keep theirs, so instances grow without merging.  It is ``distance_transform_edt(labels == 0, return_indices="linear")`` - taken on
    the labels themselves, no inverted copy is made - followed by a gather.

    On the exact path (``sampling=None``) the test is ``squared distance <= floor(distance^2)``, in integers.  With ``sampling`` it is
    ``float32 distance <= float32(distance)``.  A ``distance`` beyond every distance of the volume grows into
    all of the background.  BETWEEN TWO LABELS AT THE SAME DISTANCE the one whose nearest voxel is raster-first (smallest
    linear index) wins - scikit-image inherits SciPy's choice there.  A volume without any label comes back all zeros.

    The transform's three launches and a few element-wise torch ops over the linear index; nothing is read back, the call can be captured.
    ``distance`` negative, NaN or infinite raises ``ValueError``; the other refusals are those of ``label_distance``."""
    if labels.dtype != torch.int32:
        raise NotImplementedError(f"biapy_amd.prepost.expand_labels works on the int32 labels of label() (got {labels.dtype})")
    try:
        d = float(distance)
    except (TypeError, ValueError):
        d = float("nan")
    if not (math.isfinite(d) and d >= 0.0):
        raise ValueError(f"biapy_amd.prepost.expand_labels: distance must be a finite number >= 0 (got {distance!r})")
    dist, idx = _edt(labels, "expand_labels", False, sampling, sampling is None, indices=True, invert=True)
    if sampling is None:
        take = dist <= min(math.floor(min(d, 46341.0) ** 2), 2 ** 31 - 2)   # 46341^2 passes every finite value; below the sentinel of a volume without labels
    else:
        take = dist <= float(np.float32(min(d, 3.0e38)))              # finite in float32: below the +inf of a volume without labels
    near = _nearest_label(labels, idx)
    return torch.where(take, near, torch.zeros_like(near))


def voronoi_on_mask(labels: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """The reference's "Voronoi on mask" post-processing: every voxel with ``mask != 0`` gets the label of its nearest labelled voxel (its own if
    it has one), voxels outside the mask get 0.  ``labels``: 2-D / 3-D ``int32``; ``mask``: ``uint8`` / ``bool`` of the same shape (else
    ``ValueError``).  Nearest on the unit grid, exactly; between two labels at the same distance the one whose nearest voxel is raster-first
    wins.  A label volume without any label gives all zeros.  Returns a NEW ``int32`` tensor; nothing is read back, the call can be captured.
    The other refusals are those of ``label_distance``."""
    if labels.dtype != torch.int32:
        raise NotImplementedError(f"biapy_amd.prepost.voronoi_on_mask works on the int32 labels of label() (got {labels.dtype})")
    if mask.dtype not in (torch.uint8, torch.bool):
        raise NotImplementedError(f"biapy_amd.prepost.voronoi_on_mask works on uint8 or bool masks (got {mask.dtype})")
    if mask.shape != labels.shape:
        raise ValueError(f"biapy_amd.prepost.voronoi_on_mask: labels and mask differ in shape ({tuple(labels.shape)} and {tuple(mask.shape)})")
    if labels.is_cuda and mask.device != labels.device:
        raise RuntimeError("biapy_amd.prepost runs on the MI355X only (mask is on %s, labels on %s); there is no CPU path" % (mask.device, labels.device))
    _, idx = _edt(labels, "voronoi_on_mask", False, None, True, distances=False, indices=True, invert=True)
    near = _nearest_label(labels, idx)
    return torch.where(mask != 0, near, torch.zeros_like(near))


def label_distance(labels: torch.Tensor, sampling=None, squared: bool = False) -> torch.Tensor:
    """The per-instance distance map of an ``int32`` label image (``label()``'s output): for every voxel of label ``l != 0`` the Euclidean
    distance to the nearest voxel that does not carry ``l`` - another instance or the background - and 0 on the background.  Equal to
    ``out[labels == l] = scipy.ndimage.distance_transform_edt(labels == l)[labels == l]`` for every ``l``, in one call whatever the number of
    labels.  A label that fills the whole volume gets the sentinel (``INT32_MAX`` / ``+inf``).  ``sampling``, ``squared``, the result types
    and the refusals are those of ``distance_transform_edt``."""
    if labels.dtype != torch.int32:
        raise NotImplementedError(f"biapy_amd.prepost.label_distance works on the int32 labels of label() (got {labels.dtype})")
    return _edt(labels, "label_distance", True, sampling, squared)


# ---- seeded watershed (csrc/watershed.hip) ------------------------------------------------------------------------------------------------
# The step label() and the distance transform lead up to in the instance workflow of the reference: the seeds and the distance / probability map
# go into skimage.segmentation.watershed(image, markers, mask=foreground) on the host there.  Not offered: scikit-image's tie-breaking,
# compactness, watershed_line, an unseeded watershed from local minima, and the watershed_by_channels threshold logic around the call.

def watershed(image: torch.Tensor, markers: torch.Tensor, mask: Optional[torch.Tensor] = None, connectivity: int = 1, return_rounds: bool = False):
    """Marker-controlled watershed of a 2-D / 3-D ``float32`` or ``int32`` device tensor: an ``int32`` tensor of ``image``'s shape in which every
    voxel inside ``mask`` carries the label of the marker whose basin it falls into, 0 where no marker reaches it and outside the mask.
    ``markers``: the ``int32`` of ``label()`` (same shape); ``mask``: ``uint8`` / ``bool`` of the same shape, or ``None`` for every voxel.
    The call shape of ``skimage.segmentation.watershed(image, markers, mask=mask, connectivity=connectivity)``, with semantics of its own,
    stated exactly and checked against a host twin (``tests/watershed_ref.py``):

    * nodes are the voxels where ``mask != 0``; edges join two nodes that are neighbours at ``connectivity`` (1 faces, 2 + edges, 3 + corners,
      as ``label``; at most the tensor's rank);
    * the weight of an edge is ``max(k(u), k(v))``, ``k`` the order-preserving ``uint32`` image of the voxel's value (``int32``: ``v + 2^31``;
      ``float32``: the sign-flip map, so ``-0.0 < +0.0``; NaN is unspecified);
    * the edges are in a strict total order: (weight, linear index of the edge's raster-first endpoint ``u``, rank of the offset among ``u``'s
      forward offsets in ``(dz, dy, dx)`` lexicographic order);
    * a voxel with ``markers > 0`` inside the mask carries that label; markers <= 0 and markers outside the mask are ignored;
    * the result is the unique minimum spanning forest of this graph in which every tree holds at most one seeded group - the minimum spanning
      tree of the graph with all seeded voxels tied to one virtual root by edges below every other, minus the root; it is unique because the
      order is strict.  Every masked voxel takes the label of its tree.

    So every voxel goes to a seed that reaches it over the lowest pass height: the flooding watershed, the "watershed cut".  Seeds with the same
    label need not touch.  TIES OF THE IMAGE GO TO THE RASTER-FIRST EDGE, not to the older heap entry as in scikit-image: a perfectly flat
    plateau between two seeds is NOT split in the middle (a flat line of 21 voxels with seeds at both ends: 20 go to the first seed).  The recipe
    for saturated maps is an ``int32`` image ``(q << 15) | min(d, 32767)`` with ``q`` the quantised value and ``d`` a distance to the nearest
    marker (``distance_transform_edt(markers == 0, squared=True)`` serves): it splits plateaus along the markers' Voronoi boundary (the same
    line: 11 / 10).  ``voronoi_on_mask(markers, mask)`` gives that Voronoi split itself, as labels.

    Boruvka rounds on ``label``'s union-find (``csrc/watershed.hip``): ``4 R + 3`` launches with ``R = ceil(log2(max(n, 2))) + 1``, fixed by the
    shape and the connectivity; the rounds after the last one that joined anything return at once.  Nothing is read back, two runs give the same
    bits, the call can be captured in a graph.  ``return_rounds`` adds the number of rounds that did work as a 0-d ``int32`` DEVICE tensor.
    The workspace is 12 bytes per voxel (about 12.9 GB at 1024^3) beside the ``int32`` result.

    Refused before anything is launched: a CPU tensor (``RuntimeError``); other dtypes, an empty axis and 2^31 voxels or more
    (``NotImplementedError``); other ranks, shapes that differ and a connectivity outside ``1..ndim`` (``ValueError``)."""
    if image.dtype not in (torch.float32, torch.int32):
        raise NotImplementedError(f"biapy_amd.prepost.watershed works on float32 or int32 images (got {image.dtype})")
    if markers.dtype != torch.int32:
        raise NotImplementedError(f"biapy_amd.prepost.watershed works on the int32 markers of label() (got {markers.dtype})")
    if mask is not None and mask.dtype not in (torch.uint8, torch.bool):
        raise NotImplementedError(f"biapy_amd.prepost.watershed works on uint8 or bool masks (got {mask.dtype}); binarize() makes one")
    if image.dim() not in (2, 3):
        raise ValueError(f"biapy_amd.prepost.watershed takes a 2-D (Y, X) or 3-D (Z, Y, X) tensor (got {image.dim()} dimensions)")
    if markers.shape != image.shape or (mask is not None and mask.shape != image.shape):
        raise ValueError(f"biapy_amd.prepost.watershed: image, markers and mask must have the same shape (got {tuple(image.shape)}, {tuple(markers.shape)}"
                         + ("" if mask is None else f", {tuple(mask.shape)}") + ")")
    c = int(connectivity)
    if not 1 <= c <= image.dim():
        raise ValueError(f"connectivity must be in 1..{image.dim()} for a {image.dim()}-D image (got {connectivity})")
    for t in (image, markers) + (() if mask is None else (mask,)):
        if not t.is_cuda:
            raise RuntimeError("biapy_amd.prepost runs on the MI355X only (tensor is on %s); there is no CPU path" % t.device)
    Z, Y, X = _label_volume(image, "watershed")
    need = int(lib.bpx_watershed_workspace(Z, Y, X))
    if need < 0:
        raise NotImplementedError(f"biapy_amd.prepost.watershed: a {tuple(image.shape)} volume is refused (an empty axis, or 2^31 voxels or more)")
    img, mk = image.contiguous(), markers.contiguous()
    m = None if mask is None else mask.contiguous()
    if m is not None and m.dtype == torch.bool:
        m = m.view(torch.uint8)
    ws = torch.empty(need, dtype=torch.uint8, device=img.device)
    out = torch.empty(image.shape, dtype=torch.int32, device=img.device)
    rounds = torch.empty((), dtype=torch.int32, device=img.device)
    L.check(lib.bpx_watershed(img.data_ptr(), L.F32 if img.dtype == torch.float32 else L.I32, mk.data_ptr(), L.ptr(m), Z, Y, X, c, out.data_ptr(),
                              rounds.data_ptr(), ws.data_ptr(), need, L.stream_ptr()))
    return (out, rounds) if return_rounds else out


# ---- sparse overlap table of two label volumes and the instance matcher on top of it (csrc/overlap.hip) -----------------------------------------
# What judges the instances the steps above produce: the reference's biapy/utils/matching.py (the StarDist matcher) builds a dense
# (1 + max_true) x (1 + max_pred) overlap matrix in a host loop, turns it into IoU and runs scipy's linear_sum_assignment over all of it.  Here
# the table is sparse and built on the device; only its K rows come back.  Not offered: the criteria "iot" / "iop", report_matches and
# matching_dataset's aggregation over images; instance merging across chunk faces is LabelStitcher(rule="contact"), which counts the two faces with label_overlap.

def _overlap_inputs(a: torch.Tensor, b: torch.Tensor, max_pairs, what: str):
    for t in (a, b):
        if t.dtype != torch.int32:
            raise NotImplementedError(f"biapy_amd.prepost.{what} works on the int32 labels of label() / watershed() (got {t.dtype})")
    if a.shape != b.shape:
        raise ValueError(f"biapy_amd.prepost.{what}: the two label tensors must have the same shape (got {tuple(a.shape)}, {tuple(b.shape)})")
    if a.dim() < 1:
        raise ValueError(f"biapy_amd.prepost.{what} takes tensors of rank 1 or more (got a 0-d tensor)")
    if max_pairs is not None and int(max_pairs) < 1:
        raise ValueError(f"max_pairs must be at least 1 (got {max_pairs})")
    n = a.numel()
    if n < 1 or n >= 2 ** 31:
        raise NotImplementedError(f"biapy_amd.prepost.{what}: {n} voxels - empty volumes and volumes of 2^31 voxels or more are not supported")
    mp = min(n, 2 ** 21) if max_pairs is None else int(max_pairs)
    need = int(lib.bpx_overlap_workspace(mp))
    if need < 0:
        raise NotImplementedError(f"biapy_amd.prepost.{what}: max_pairs = {mp} is refused (the table would pass 2^31 slots)")
    for t in (a, b):
        if not t.is_cuda:
            raise RuntimeError("biapy_amd.prepost runs on the MI355X only (tensor is on %s); there is no CPU path" % t.device)
    return mp, need


def label_overlap(a: torch.Tensor, b: torch.Tensor, max_pairs: Optional[int] = None):
    """The sparse contingency table of two ``int32`` label tensors of the same shape (any rank >= 1; views are taken via ``.contiguous()``): every
    distinct pair ``(a[i], b[i])`` with the number of voxels that carry it, the pairs with background included.  A label ``<= 0`` counts as
    background 0, as ``watershed`` treats its markers.  Returns ``(pairs, counts, num)``:

    * ``pairs``: ``int32`` of shape ``(max_pairs, 2)``, SORTED by ``(a, b)``; the rows from ``num`` onward are ``(-1, -1)``;
    * ``counts``: ``int32`` of shape ``(max_pairs,)``, 0 from ``num`` onward;
    * ``num``: the number ``K`` of distinct pairs as a 0-d ``int32`` DEVICE tensor, ``-1`` when there are more than ``max_pairs`` of them (the
      other two results are then unspecified).

    ``pairs[:K]`` / ``counts[:K]`` equal ``np.unique`` (with counts) of the packed keys ``a << 32 | b`` bit for bit.  ``max_pairs`` defaults to
    ``min(n, 2**21)``: the table has the power of two ``>= 2 * max_pairs`` slots of 12 bytes, 48 MB at the default.  Three launches fixed by
    ``(n, max_pairs)`` and one ``torch.sort`` of the fixed-size key array: nothing is read back, two runs give the same bits, the call can be
    captured in a graph.

    Refused before anything is launched: a CPU tensor (``RuntimeError``); other dtypes, an empty tensor, 2^31 voxels or more and a ``max_pairs``
    whose table would pass 2^31 slots (``NotImplementedError``); shapes that differ and ``max_pairs < 1`` (``ValueError``)."""
    mp, need = _overlap_inputs(a, b, max_pairs, "label_overlap")
    fa, fb = a.contiguous(), b.contiguous()
    ws = torch.empty(need, dtype=torch.uint8, device=fa.device)
    keys = torch.empty(mp, dtype=torch.int64, device=fa.device)
    counts = torch.empty(mp, dtype=torch.int32, device=fa.device)
    num = torch.empty((), dtype=torch.int32, device=fa.device)
    L.check(lib.bpx_label_overlap(fa.data_ptr(), fb.data_ptr(), fa.numel(), mp, keys.data_ptr(), counts.data_ptr(), num.data_ptr(), ws.data_ptr(),
                                  need, L.stream_ptr()))
    keys, order = torch.sort(keys)                       # the keys are distinct but for the INT64_MAX filler, whose counts are all 0
    counts = counts[order]
    filler = keys == torch.iinfo(torch.int64).max
    pairs = torch.stack((keys >> 32, keys & 0xFFFFFFFF), dim=1).masked_fill(filler[:, None], -1).to(torch.int32)
    return pairs, counts, num


def _safe_divide(x: float, y: float, eps: float = 1e-10) -> float:
    return x / y if abs(y) > eps else 0.0


def _match_stats(pairs, counts, thresh):
    """The reference's ``matching()`` (criterion "iou") from the sparse overlap table alone - a pure host function, no tensors: ``pairs`` (K, 2)
    label pairs with background 0, ``counts`` (K,) voxels per pair, ``thresh`` one threshold.  Areas are the row and column sums of the table;
    ``n_true`` / ``n_pred`` the distinct positive labels present (they need not be sequential); IoU = c / (|a| + |b| - c) in float64 over the
    positive pairs; the reference's cost ``-(iou >= thr) - iou / (2 * min(n_true, n_pred))`` is minimised with
    ``scipy.optimize.linear_sum_assignment`` PER CONNECTED BLOCK of the overlap graph: two labels that share no voxel have cost 0, no cost is
    positive, so an optimum of the dense problem is a union of optima of the blocks and the dense matrix over all labels is never built."""
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError as e:
        raise ImportError("biapy_amd.prepost.matching needs scipy (scipy.optimize.linear_sum_assignment), which is not installed") from e
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    thr = float(thresh)
    ut, it = np.unique(pairs[:, 0], return_inverse=True)
    up, ip = np.unique(pairs[:, 1], return_inverse=True)
    area_t, area_p = np.zeros(ut.size, np.int64), np.zeros(up.size, np.int64)
    np.add.at(area_t, it, c)
    np.add.at(area_p, ip, c)
    n_true, n_pred = int((ut > 0).sum()), int((up > 0).sum())
    n_matched = min(n_true, n_pred)
    pos = (pairs[:, 0] > 0) & (pairs[:, 1] > 0) & (c > 0)
    rows, cols, cc = it[pos], ip[pos], c[pos]
    iou = cc.astype(np.float64) / (area_t[rows] + area_p[cols] - cc).astype(np.float64)
    tp, sum_matched = 0, 0.0
    if n_matched > 0 and iou.size and bool((iou >= thr).any()):
        # connected blocks of the bipartite overlap graph: union-find over (true rows, pred columns), path halving
        parent = np.arange(ut.size + up.size)

        def find(i):
            while parent[i] != i:
                parent[i] = parent[parent[i]]
                i = parent[i]
            return i

        for r, q in zip(rows.tolist(), (cols + ut.size).tolist()):
            ra, rb = find(r), find(q)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
        block = np.array([find(r) for r in rows.tolist()])
        for root in np.unique(block[iou >= thr]):        # a block without a pair at the threshold holds no match that counts
            sel = block == root
            br, bq, bi = rows[sel], cols[sel], iou[sel]
            lr, jr = np.unique(br, return_inverse=True)
            lq, jq = np.unique(bq, return_inverse=True)
            score = np.zeros((lr.size, lq.size), np.float64)
            score[jr, jq] = bi
            cost = -(score >= thr).astype(np.float64) - score / (2 * n_matched)
            ti, pi = linear_sum_assignment(cost)
            ok = score[ti, pi] >= thr
            tp += int(np.count_nonzero(ok))
            sum_matched += float(np.sum(score[ti, pi][ok]))
    fp, fn = n_pred - tp, n_true - tp
    return dict(criterion="iou", thresh=thresh, fp=fp, tp=tp, fn=fn,
                precision=tp / (tp + fp) if tp > 0 else 0, recall=tp / (tp + fn) if tp > 0 else 0,
                accuracy=tp / (tp + fp + fn) if tp > 0 else 0, f1=(2 * tp) / (2 * tp + fp + fn) if tp > 0 else 0,
                n_true=n_true, n_pred=n_pred, mean_true_score=_safe_divide(sum_matched, n_true), mean_matched_score=_safe_divide(sum_matched, tp),
                panoptic_quality=_safe_divide(sum_matched, tp + fp / 2 + fn / 2))


def matching(y_true: torch.Tensor, y_pred: torch.Tensor, thresh=0.5, criterion: str = "iou", max_pairs: Optional[int] = None):
    """The reference's ``matching(y_true, y_pred, thresh, criterion)`` (``biapy/utils/matching.py``, the StarDist matcher) on two ``int32`` label
    tensors that stay on the device: a dict with the reference's keys - ``criterion, thresh, fp, tp, fn, precision, recall, accuracy, f1, n_true,
    n_pred, mean_true_score, mean_matched_score, panoptic_quality`` - or, for a sequence of thresholds, a list of them.  ``label_overlap`` builds
    the sparse table on the device, its ``K`` rows (kilobytes) are read back, the assignment is solved on the host per connected block of the
    overlap graph (``_match_stats``).  Labels need not be sequential; an empty ``y_true`` or ``y_pred`` gives the reference's zeros.

    Only ``criterion="iou"`` is offered (others raise ``NotImplementedError``).  More than ``max_pairs`` distinct pairs (default
    ``min(n, 2**21)``) raise ``RuntimeError``: call again with a larger ``max_pairs``.  The refusals of ``label_overlap`` apply; ``scipy`` is
    imported here, not with the package, and its absence raises ``ImportError``."""
    if criterion != "iou":
        raise NotImplementedError(f"biapy_amd.prepost.matching offers criterion 'iou' only (got {criterion!r})")
    mp, _ = _overlap_inputs(y_true, y_pred, max_pairs, "matching")
    pairs, counts, num = label_overlap(y_true, y_pred, mp)
    k = int(num)
    if k < 0:
        raise RuntimeError(f"biapy_amd.prepost.matching: the two volumes hold more than max_pairs = {mp} distinct label pairs; pass a larger max_pairs")
    p, c = pairs[:k].cpu().numpy(), counts[:k].cpu().numpy()
    if np.isscalar(thresh):
        return _match_stats(p, c, thresh)
    return [_match_stats(p, c, t) for t in thresh]


# ---- region properties of a label volume and the property filter on top of them (csrc/regionprops.hip) -------------------------------------------
# What every consumer of label() / watershed() does next: the detection workflow takes the centroids of its labelled blobs, the instance workflow
# measures every instance and drops those that fail a property test, and a crop of an instance needs its box (skimage.measure.regionprops,
# scipy.ndimage.find_objects / center_of_mass on the host there).  Offered: area, bbox, the exact coordinate sums and the centroid; second
# moments, voxel faces, the 2-D perimeter and the measures derived from them are shape_props, below; minimum, maximum, exact sum and mean of
# an image over every label are intensity_props, further below.  NOT offered: intensity_std and the weighted moments; a meshed surface; coords,
# image, convex_*; volumes of 2^31 voxels or more; multi-GPU slabs.

class RegionProps(NamedTuple):
    """``region_props``' result, every field a device tensor with one row per label ``0..N``; row 0 is the background's and holds zeros (NaN in
    ``centroid``), as does the row of a label that no voxel carries."""
    area: torch.Tensor        # int32 (N + 1,)
    bbox: torch.Tensor        # int32 (N + 1, 2 * ndim): (z0, y0, x0, z1, y1, x1) half-open, (y0, x0, y1, x1) in 2-D
    coord_sum: torch.Tensor   # int64 (N + 1, ndim): the sums of the voxels' coordinates, exact
    centroid: torch.Tensor    # float64 (N + 1, ndim): coord_sum / area, NaN where area == 0


def region_props(labels: torch.Tensor, num=None) -> RegionProps:
    """Area, bounding box and centroid of every label ``1..N`` of a 2-D ``(Y, X)`` or 3-D ``(Z, Y, X)`` ``int32`` label tensor, as a
    ``RegionProps`` named tuple of DEVICE tensors: ``area`` equals ``np.bincount`` (``component_sizes``) from row 1 on, ``bbox`` is scikit-image's
    ``regionprops`` ``bbox`` (the slices of ``scipy.ndimage.find_objects``, half-open), ``coord_sum`` the exact integer sums of the coordinates
    and ``centroid = coord_sum.double() / area.double()`` (scikit-image's ``centroid``, ``scipy.ndimage.center_of_mass`` of the label), NaN where
    ``area == 0``.  The three integer results are bit for bit the same on every run.  Voxels with a label ``<= 0`` or ``> N`` contribute nothing.

    ``num``: ``N`` as a Python int (no wait for the device; inside a graph an upper bound serves, the rows past the labels present are zeros), or
    the 0-d tensor of ``label(..., return_num=True)``, which is read back here; ``None`` reads ``labels.max()`` back, as ``remove_small_objects``
    does.  Views are taken via ``.contiguous()``.  Three launches fixed by the shape and ``N``, nothing else read back: capturable.

    Refused before anything is launched: a negative ``num`` and a rank other than 2 / 3 (``ValueError``); a CPU tensor (``RuntimeError``); a dtype
    other than ``int32``, an empty volume and 2^31 voxels or more (``NotImplementedError``).  Second moments, faces and the 2-D perimeter:
    ``shape_props``; minimum, maximum, sum and mean of an image: ``intensity_props``.  Not offered: ``intensity_std``, ``coords`` / ``image`` /
    ``convex_*``, multi-GPU slabs (see the comment above)."""
    n_max = None if num is None else int(num)
    if n_max is not None and n_max < 0:
        raise ValueError(f"num must not be negative (got {n_max})")
    Z, Y, X = _label_volume(labels, "region_props")
    lab = _labels(labels, "region_props").contiguous()
    if n_max is None:
        n_max = max(int(lab.max()), 0)
    area = torch.empty(n_max + 1, dtype=torch.int32, device=lab.device)
    sums = torch.empty((n_max + 1, 3), dtype=torch.int64, device=lab.device)
    bbox = torch.empty((n_max + 1, 6), dtype=torch.int32, device=lab.device)
    L.check(lib.bpx_region_props(lab.data_ptr(), Z, Y, X, n_max, area.data_ptr(), sums.data_ptr(), bbox.data_ptr(), L.stream_ptr()))
    if labels.dim() == 2:                                   # Z = 1: the z columns are all zeros (and ones)
        sums, bbox = sums[:, 1:], bbox[:, [1, 2, 4, 5]]
    return RegionProps(area, bbox, sums, sums.double() / area.double()[:, None])


def centroids(labels: torch.Tensor, num=None) -> torch.Tensor:
    """The centroids of the labels ``1..N`` as a ``float64`` device tensor of shape ``(N, ndim)`` - ``region_props(labels, num).centroid[1:]``,
    what the detection workflow takes from its labelled blobs; NaN for a label that no voxel carries."""
    return region_props(labels, num).centroid[1:]


def instance_targets(labels: torch.Tensor, channels=("F", "C", "D"), num=None, **options) -> torch.Tensor:
    """The instance-segmentation channel targets of ONE 2-D ``(Y, X)`` or 3-D ``(Z, Y, X)`` ``int32`` label tensor as a ``float32`` device tensor
    ``(Ct, [Z,] Y, X)`` - the offline target generation the reference does with SciPy on the host, and ``biapy_amd.targets.InstanceTargets`` at a
    batch of one: its channels (``F``, ``C``, ``D``, ``Dc``, ``H``, ``V``, ``Z``), its ``options`` (``contour_mode``, ``contour_connectivity``,
    ``f_excludes_contour``, ``d_norm``, ``d_clip``, ``sampling``), its arithmetic and its refusals; the semantics are stated there.  ``num`` as for
    ``region_props`` (an int, the 0-d tensor of ``label(..., return_num=True)``, or ``None``, which reads ``labels.max()`` back); it must stay
    below 2^24.  A label ``<= 0`` or ``> num`` is background.  Known limit: the records pass reads the distances of a run (the voxels of one
    label along a row) through one lane, so a volume whose rows stay inside one label for thousands of voxels pays for it; it is sized for and
    measured at training patches, not at such volumes."""
    from .targets import InstanceTargets, _check_channels

    if "augment" in options or "n_max" in options:
        raise ValueError("biapy_amd.prepost.instance_targets takes num= and no augmenter")
    channels = _check_channels(channels)
    n_max = None if num is None else int(num)
    if n_max is not None and n_max < 0:
        raise ValueError(f"num must not be negative (got {n_max})")
    _label_volume(labels, "instance_targets")
    lab = _labels(labels, "instance_targets").contiguous()
    if n_max is None:
        n_max = max(int(lab.max()), 0)
    return InstanceTargets(channels, n_max=n_max, **options)(None, lab[None])[1][0]


def select_objects(labels: torch.Tensor, keep: torch.Tensor, relabel: bool = False, return_num: bool = False):
    """The general form of ``remove_small_objects``: a NEW ``int32`` label tensor in which every label ``l`` with ``keep[l]`` false is 0.  ``keep``
    is a ``bool`` or ``uint8`` device tensor of length ``N + 1`` (entry 0, the background's, is ignored), typically a torch expression over the
    tensors of ``region_props``: ``p.area >= 64``; ``(p.bbox[:, :3] > 0).all(1) & (p.bbox[:, 3:] < shape).all(1)`` for "does not touch the
    border"; a ratio of box extents.  The survivors keep their ids; ``relabel=True`` renumbers them ``1..N'`` in the same order.  Labels above
    ``N = len(keep) - 1`` become 0, as ``remove_small_objects`` treats labels above ``num``; a kept id that no voxel carries counts as a survivor.
    ``return_num`` adds ``N'``, the number of survivors, as a 0-d ``int32`` device tensor.  Two launches, nothing read back: capturable."""
    if keep.dtype not in (torch.bool, torch.uint8):
        raise NotImplementedError(f"biapy_amd.prepost.select_objects: keep must be a bool or uint8 tensor (got {keep.dtype})")
    if keep.dim() != 1 or keep.numel() < 1:
        raise ValueError(f"biapy_amd.prepost.select_objects: keep must have shape (N + 1,) (got {tuple(keep.shape)})")
    if not keep.is_cuda:
        raise RuntimeError("biapy_amd.prepost.select_objects: keep must be on the device (it is on %s); there is no CPU path" % keep.device)
    lab = _labels(labels, "select_objects")
    n_max = keep.numel() - 1
    sizes = (keep != 0).to(torch.int32)                     # bpx_label_filter with min_size 1: "size" 1 survives, 0 does not
    sizes[:1].zero_()                                       # a fill, not a copy from the host: capturable
    out = lab.clone(memory_format=torch.contiguous_format)
    left = torch.empty((), dtype=torch.int32, device=lab.device)
    L.check(lib.bpx_label_filter(out.data_ptr(), out.numel(), n_max, sizes.data_ptr(), 1, 1 if relabel else 0, left.data_ptr(), L.stream_ptr()))
    return (out, left) if return_num else out


# ---- shape properties: second moments, voxel faces, the 2-D perimeter, and the measures derived from them (csrc/shapeprops.hip) --------------------
# The rest of the reference's property filter (circularity, elongation, perimeter, sphericity beside npixels / area / diameter).  All of it is
# integer sums reached by commutative atomics, so "the same bits every run" holds; the derived measures are plain torch expressions over the
# fields - no solver library, nothing read back - and each of them, or any other expression, feeds ``select_objects``.

class ShapeProps(NamedTuple):
    """``shape_props``' result, every field a device tensor with one row per label ``0..N``; row 0 and the row of a label that no voxel carries
    hold zeros (NaN in ``centroid``).  The first four fields are ``RegionProps``'."""
    area: torch.Tensor                          # int32 (N + 1,)
    bbox: torch.Tensor                          # int32 (N + 1, 2 * ndim)
    coord_sum: torch.Tensor                     # int64 (N + 1, ndim)
    centroid: torch.Tensor                      # float64 (N + 1, ndim)
    moments: torch.Tensor                       # int64 (N + 1, 6): the sums of zz, yy, xx, zy, zx, yx, exact; (N + 1, 3) in 2-D: yy, xx, yx
    covariance: torch.Tensor                    # float64 (N + 1, ndim, ndim): moments / area - centroid centroid^T, from the exact numerator
    faces: torch.Tensor                         # int64 (N + 1, ndim): voxel faces towards another label or the outside, per axis
    perimeter_classes: Optional[torch.Tensor]   # int32 (N + 1, 3) in 2-D: pixels of weight 1, sqrt 2, (1 + sqrt 2) / 2; None in 3-D


_COV_3D = ((0, 3, 4), (3, 1, 5), (4, 5, 2))     # covariance[i][j] = column of bpx_region_moments' cov_d
_COV_2D = ((1, 5), (5, 2))


def _columns(t: torch.Tensor, which) -> torch.Tensor:
    """``t[:, which]`` without an index tensor, which would be copied from the host and cannot be captured."""
    return torch.stack([t[:, c] for c in which], 1)


def moments_fit(shape) -> bool:
    """Whether ``shape_props`` accepts a volume of this shape: ``n * (Emax - 1)**2 < 2**63`` (``n`` the voxel count, ``Emax`` the largest
    extent), under which every second-order coordinate sum fits ``int64``.  Every volume below 2^31 voxels with no extent above 65 536 passes, a single row up to 2^21 voxels (2^15 rows of 2^16 do, of 2^17 do not)."""
    n, emax = math.prod(shape), max(shape)
    return n * (emax - 1) ** 2 < 2 ** 63


def shape_props(labels: torch.Tensor, num=None) -> ShapeProps:
    """``region_props`` plus the exact second-order coordinate sums, the covariance matrix, the voxel faces per axis and (2-D) the weight classes
    of scikit-image's perimeter estimator of every label ``1..N`` of a 2-D ``(Y, X)`` or 3-D ``(Z, Y, X)`` ``int32`` label tensor, as a
    ``ShapeProps`` named tuple of DEVICE tensors.  Every integer field is bit for bit the same on every run; ``covariance`` follows from the
    integers by a fixed sequence of float64 operations (the exact 128-bit numerator ``A * S_ab - S_a * S_b``, converted, divided by ``A``
    twice).  ``faces[l][k]`` counts the (voxel of ``l``, direction along axis ``k``) pairs whose neighbour carries another label or lies outside.

    ``num`` as for ``region_props``.  Launches fixed by the shape and ``N`` (``bpx_region_props``, ``bpx_region_moments``, ``bpx_region_faces``
    and, in 2-D, ``bpx_region_perimeter2d``), nothing else read back: capturable.  Refused before anything is launched, in this order: what
    ``region_props`` refuses up to the voxel count; a shape with ``n * (Emax - 1)**2 >= 2**63`` (``NotImplementedError``, ``moments_fit``);
    then its dtype, device and empty-volume refusals.  Intensities: ``intensity_props``.  Not offered: ``coords`` / ``image`` / ``convex_*``, multi-GPU slabs.

    The measures on top - ``principal_moments``, ``axis_lengths``, ``elongation``, ``surface_area``, ``perimeter``, ``circularity``,
    ``sphericity`` - are torch expressions of one row per label; ``select_objects(labels, elongation(p) < 3)`` filters by them."""
    n_max = None if num is None else int(num)
    if n_max is not None and n_max < 0:
        raise ValueError(f"num must not be negative (got {n_max})")
    Z, Y, X = _label_volume(labels, "shape_props")
    if not moments_fit((Z, Y, X)):
        raise NotImplementedError(f"biapy_amd.prepost.shape_props: a {Z} x {Y} x {X} volume has n * (Emax - 1)^2 >= 2^63 - its second-order "
                                  "coordinate sums may not fit int64")
    lab = _labels(labels, "shape_props").contiguous()
    if n_max is None:
        n_max = max(int(lab.max()), 0)
    dev, rows, two_d = lab.device, n_max + 1, labels.dim() == 2
    area = torch.empty(rows, dtype=torch.int32, device=dev)
    sums = torch.empty((rows, 3), dtype=torch.int64, device=dev)
    bbox = torch.empty((rows, 6), dtype=torch.int32, device=dev)
    mom = torch.empty((rows, 6), dtype=torch.int64, device=dev)
    cov = torch.empty((rows, 6), dtype=torch.float64, device=dev)
    faces = torch.empty((rows, 3), dtype=torch.int64, device=dev)
    s = L.stream_ptr()
    L.check(lib.bpx_region_props(lab.data_ptr(), Z, Y, X, n_max, area.data_ptr(), sums.data_ptr(), bbox.data_ptr(), s))
    L.check(lib.bpx_region_moments(lab.data_ptr(), Z, Y, X, n_max, area.data_ptr(), sums.data_ptr(), mom.data_ptr(), cov.data_ptr(), s))
    L.check(lib.bpx_region_faces(lab.data_ptr(), Z, Y, X, n_max, faces.data_ptr(), s))
    classes = None
    if two_d:
        classes = torch.empty((rows, 3), dtype=torch.int32, device=dev)
        L.check(lib.bpx_region_perimeter2d(lab.data_ptr(), Y, X, n_max, classes.data_ptr(), s))
        sums, bbox, mom, faces = sums[:, 1:], _columns(bbox, (1, 2, 4, 5)), _columns(mom, (1, 2, 5)), faces[:, 1:]
    cov = _columns(cov, [c for row in (_COV_2D if two_d else _COV_3D) for c in row]).reshape(rows, labels.dim(), labels.dim())
    return ShapeProps(area, bbox, sums, sums.double() / area.double()[:, None], mom, cov, faces, classes)


# ---- intensity properties: exact sum, mean, min, max of an image over every label (csrc/intensityprops.hip) -----------------------------------------
# The one per-label measurement with a second volume-sized operand: the mean foreground probability of an instance as its confidence, the mean /
# minimum / maximum raw intensity of a cell (skimage's intensity_mean / intensity_min / intensity_max, scipy.ndimage.mean / minimum / maximum
# with an index, on the host there).  "The same bits every run" holds: min / max are integer atomics on an order-preserving key, and the sum is
# kept EXACTLY in int64 limbs of a fixed-point line (integer adds commute) and rounded once.  NOT offered: intensity_std or any second moment of
# a float32 image (the exact product needs 18 limbs - a named follow-up); centroid_weighted and the weighted moments; multi-channel images; int32,
# float64 or 16-bit float images; percentiles per label; volumes of 2^31 voxels or more; multi-GPU slabs.

class IntensityProps(NamedTuple):
    """``intensity_props``' result, every field a device tensor with one row per label ``0..N``; row 0 and the row of a label that no voxel
    carries hold zeros (NaN in ``mean``)."""
    area: torch.Tensor        # int32 (N + 1,): equals region_props(...).area bit for bit
    min: torch.Tensor         # (N + 1,) float32 for a float32 image, int32 for uint8 / uint16
    max: torch.Tensor         # likewise
    sum: torch.Tensor         # float64 (N + 1,): the exact sum, rounded once (to nearest even)
    mean: torch.Tensor        # float64 (N + 1,): sum / area, one IEEE division; NaN where area == 0
    sum_limbs: torch.Tensor   # int64 (N + 1, NL): NL = 9 for float32 (unit 2^-149), 1 for uint8 / uint16 (unit 1)
    nonfinite: torch.Tensor   # int32 (N + 1, 3): the numbers of NaN, +inf, -inf voxels (zeros for integer images)


_INTENSITY_DTYPES = {torch.float32: (L.F32, 9, torch.float32), torch.uint8: (L.U8, 1, torch.int32)}
if hasattr(torch, "uint16"):
    _INTENSITY_DTYPES[torch.uint16] = (L.U16, 1, torch.int32)


def intensity_props(labels: torch.Tensor, image: torch.Tensor, num=None) -> IntensityProps:
    """Count, minimum, maximum, EXACT sum and mean of ``image`` over every label ``1..N`` of a 2-D ``(Y, X)`` or 3-D ``(Z, Y, X)`` ``int32``
    label tensor, as an ``IntensityProps`` named tuple of DEVICE tensors.  ``image`` has the labels' shape and is ``float32``, ``uint8`` or
    ``torch.uint16``.  Every field but ``mean`` is bit for bit the same on every run, and ``mean`` follows from two of them by one division.

    ``sum_limbs[l, j]`` is the sum, over the finite voxels of label ``l``, of that voxel's piece for limb ``j``: with ``bits`` the voxel's
    ``float32`` word, ``E = (bits >> 23) & 255`` and ``f = bits & 0x7fffff``, ``(m, q) = (f, 0)`` if ``E == 0`` else ``(f | 0x800000, E - 1)``,
    ``w = m << (q & 31)``; the piece for limb ``q >> 5`` is ``w & 0xffffffff``, the piece for limb ``(q >> 5) + 1`` is ``w >> 32``, both negated
    for a negative voxel.  For integer images limb 0 is the plain integer sum.  ``sum`` is the exact value ``sum_j limbs[j] * 2**(32 j - 149)``
    (unit 1 for integers) rounded ONCE to ``float64``, to nearest even - what ``math.fsum`` returns; below ``2**159`` in magnitude and, if
    nonzero, at least ``2**-149``, so it neither overflows nor underflows; an exact zero is ``+0.0``.  ``mean = sum / area`` rounds twice (the
    sum, then the division).  NaN voxels are left out of ``min``, ``max`` and ``sum_limbs``, are counted in ``nonfinite`` and make ``sum`` and
    ``mean`` NaN; a label whose voxels are all NaN has ``min = max = NaN``.  Infinite voxels take part in ``min`` and ``max``, are left out of
    the limbs and make ``sum`` that infinity, or NaN when both signs occur in the label.  ``min`` and ``max`` follow the order of the bits:
    ``-0.0 < +0.0``, and the bits of the winning voxel are returned.  Voxels with a label ``<= 0`` or ``> N`` contribute nothing.

    ``num`` as for ``region_props``: a Python int, a 0-d tensor, or ``None``, which reads ``labels.max()`` back.  Views are taken via
    ``.contiguous()``.  Three launches fixed by the shape, the dtype and ``N``, nothing else read back: capturable.
    ``select_objects(labels, p.mean >= t)`` filters instances by their mean probability.

    Refused before anything is launched, in this order: a rank other than 2 / 3, a negative ``num``, an image of another shape (``ValueError``);
    a CPU tensor or operands on two devices (``RuntimeError``); labels that are not ``int32``, an image dtype other than the three named, an
    empty volume, 2^31 voxels or more (``NotImplementedError``).  Not offered: ``intensity_std`` and other second moments, weighted centroids
    and moments, multi-channel images, ``int32`` / ``float64`` / 16-bit float images, percentiles, multi-GPU slabs (see the comment above)."""
    if labels.dim() not in (2, 3):
        raise ValueError(f"biapy_amd.prepost.intensity_props takes a 2-D (Y, X) or 3-D (Z, Y, X) tensor (got {labels.dim()} dimensions)")
    n_max = None if num is None else int(num)
    if n_max is not None and n_max < 0:
        raise ValueError(f"num must not be negative (got {n_max})")
    if tuple(image.shape) != tuple(labels.shape):
        raise ValueError(f"biapy_amd.prepost.intensity_props: the image must have the labels' shape {tuple(labels.shape)} (got {tuple(image.shape)})")
    if not labels.is_cuda or not image.is_cuda:
        raise RuntimeError("biapy_amd.prepost runs on the MI355X only (labels are on %s, the image on %s); there is no CPU path" % (labels.device, image.device))
    if labels.device != image.device:
        raise RuntimeError(f"biapy_amd.prepost.intensity_props: labels ({labels.device}) and image ({image.device}) must be on the same device")
    if labels.dtype != torch.int32:
        raise NotImplementedError(f"biapy_amd.prepost.intensity_props works on the int32 labels of label() (got {labels.dtype})")
    if image.dtype not in _INTENSITY_DTYPES:
        raise NotImplementedError(f"biapy_amd.prepost.intensity_props works on float32, uint8 or uint16 images (got {image.dtype})")
    if labels.numel() < 1:
        raise NotImplementedError("biapy_amd.prepost.intensity_props: empty volumes are not supported")
    if labels.numel() >= 2 ** 31:
        raise NotImplementedError(f"biapy_amd.prepost.intensity_props: {labels.numel()} voxels - volumes of 2^31 voxels or more are not supported")
    Z, Y, X = (1,) + tuple(labels.shape) if labels.dim() == 2 else tuple(labels.shape)
    lab, img = labels.contiguous(), image.contiguous()
    if n_max is None:
        n_max = max(int(lab.max()), 0)
    code, nl, out_dtype = _INTENSITY_DTYPES[img.dtype]
    dev, rows = lab.device, n_max + 1
    area = torch.empty(rows, dtype=torch.int32, device=dev)
    lo = torch.empty(rows, dtype=out_dtype, device=dev)
    hi = torch.empty(rows, dtype=out_dtype, device=dev)
    limbs = torch.empty((rows, nl), dtype=torch.int64, device=dev)
    nonf = torch.empty((rows, 3), dtype=torch.int32, device=dev)
    total = torch.empty(rows, dtype=torch.float64, device=dev)
    mean = torch.empty(rows, dtype=torch.float64, device=dev)
    L.check(lib.bpx_intensity_props(lab.data_ptr(), img.data_ptr(), code, Z, Y, X, n_max, area.data_ptr(), lo.data_ptr(), hi.data_ptr(), limbs.data_ptr(),
                                    nonf.data_ptr(), total.data_ptr(), mean.data_ptr(), L.stream_ptr()))
    return IntensityProps(area, lo, hi, total, mean, limbs, nonf)


def _shape_props(p, what: str) -> int:
    if not isinstance(p, ShapeProps):
        raise TypeError(f"biapy_amd.prepost.{what} takes the ShapeProps of shape_props (got {type(p).__name__})")
    return p.faces.shape[1]


def _sampling(sampling, ndim: int, what: str):
    if sampling is None:
        return (1.0,) * ndim
    s = tuple(float(v) for v in sampling)
    if len(s) != ndim or not all(math.isfinite(v) and v > 0 for v in s):
        raise ValueError(f"biapy_amd.prepost.{what}: sampling must be {ndim} finite positive numbers (got {sampling!r})")
    return s


def _eig2(a: torch.Tensor, d: torch.Tensor, b: torch.Tensor):
    """The eigenvalues of [[a, b], [b, d]], the larger first."""
    mid, half = (a + d) / 2, torch.sqrt(((a - d) / 2) ** 2 + b * b)
    return mid + half, mid - half


def principal_moments(p: ShapeProps) -> torch.Tensor:
    """The eigenvalues of ``p.covariance`` in descending order, ``float64 (N + 1, ndim)``, never negative - scikit-image's ``inertia_tensor_eigvals``.
    Closed forms, elementwise torch: no solver, nothing read back.  2-D: ``(a + d) / 2 +- sqrt(((a - d) / 2)^2 + b^2)``, a few units of
    ``2^-52 * trace``.  3-D: the trigonometric form ``q + 2 s cos(phi + 2 pi k / 3)`` with ``phi = acos(det(C - q I) / (2 s^3)) / 3``; where two
    eigenvalues nearly coincide while the third lies far off (a long thin object) the arc cosine is taken near 1 and the two close ones are only
    good to about ``1e-8 * trace`` (measured: tests/shapeprops_ref.py, profiles/shapeprops_values.txt).  An object that is flat along an axis (a
    rod, a plane one voxel thick) has an exactly zero variance there - the covariance's numerator is an exact integer - and is reduced to the 2-D
    form, so its zero eigenvalue is exact."""
    nd = _shape_props(p, "principal_moments")
    c = p.covariance
    if nd == 2:
        return torch.stack(_eig2(c[:, 0, 0], c[:, 1, 1], c[:, 0, 1]), 1).clamp_min(0)
    a, d, f = c[:, 0, 0], c[:, 1, 1], c[:, 2, 2]
    b, e, g = c[:, 0, 1], c[:, 0, 2], c[:, 1, 2]
    q = (a + d + f) / 3
    p1 = b * b + e * e + g * g
    a0, d0, f0 = a - q, d - q, f - q
    s = torch.sqrt((a0 * a0 + d0 * d0 + f0 * f0 + 2 * p1) / 6)
    det = a0 * (d0 * f0 - g * g) - b * (b * f0 - g * e) + e * (b * g - d0 * e)
    r = torch.where(s > 0, det / (2 * s * s * s), torch.zeros_like(s)).clamp(-1, 1)
    phi = torch.acos(r) / 3
    hi = q + 2 * s * torch.cos(phi)
    lo = q + 2 * s * torch.cos(phi + 2 * math.pi / 3)
    lam = torch.stack((hi, 3 * q - hi - lo, lo), 1)
    zero = torch.zeros_like(q)
    for flat, (u, v, w) in ((a == 0, (d, f, g)), (d == 0, (a, f, e)), (f == 0, (a, d, b))):        # no variance along z, y, x: the other two axes' 2 x 2
        lam = torch.where(flat[:, None], torch.stack(_eig2(u, v, w) + (zero,), 1), lam)
    return torch.sort(lam.clamp_min(0), dim=1, descending=True).values          # equal eigenvalues may come out an ulp out of order


def axis_lengths(p: ShapeProps) -> torch.Tensor:
    """The lengths of the axes of the ellipse / ellipsoid with the object's second moments, longest first: ``4 sqrt(lambda)`` in 2-D
    (scikit-image's ``axis_major_length`` / ``axis_minor_length``), ``sqrt(20 lambda)`` in 3-D."""
    lam = principal_moments(p)
    return 4 * torch.sqrt(lam) if lam.shape[1] == 2 else torch.sqrt(20 * lam)


def elongation(p: ShapeProps) -> torch.Tensor:
    """``sqrt(lambda_max / lambda_min)`` of the principal moments: 1 for a disk, ball, square or cube, ``inf`` for a flat object (a rod, a plane
    one voxel thick; in 3-D an object flat along a direction that is no axis, a diagonal line, gets a large finite value instead), NaN for a
    single voxel and for an absent label."""
    lam = principal_moments(p)
    return torch.sqrt(lam[:, 0] / lam[:, -1])


def surface_area(p: ShapeProps, sampling=None) -> torch.Tensor:
    """``sum_k faces_k * prod_{j != k} sampling_j``: the area of the object's voxel faces (in 2-D the length of its pixel edges), ``float64
    (N + 1,)``.  The face count of a digitised ball tends to 1.5 x its true surface and that of a disk to 4 / pi x its circumference (ratios
    1.4995 at r = 40 and 1.281 at r = 80): a staircase does not shorten as the grid is refined."""
    nd = _shape_props(p, "surface_area")
    s = _sampling(sampling, nd, "surface_area")
    w = [math.prod(s[j] for j in range(nd) if j != k) for k in range(nd)]          # Python floats: no copy to the device, capturable
    return sum(p.faces[:, k].double() * w[k] for k in range(nd))


_PERIMETER_WEIGHTS = (1.0, math.sqrt(2.0), (1.0 + math.sqrt(2.0)) / 2.0)


def perimeter(p: ShapeProps) -> torch.Tensor:
    """scikit-image's ``perimeter(label == l, neighborhood=4)`` of every label of a 2-D image, ``float64 (N + 1,)``: the border pixels in three
    classes by the border pixels around them, weighted 1, sqrt 2 and (1 + sqrt 2) / 2.  It follows scikit-image's estimator, not the pixel-edge
    length (``surface_area``).  3-D raises ``ValueError``."""
    if _shape_props(p, "perimeter") != 2:
        raise ValueError("biapy_amd.prepost.perimeter is defined for 2-D labels only; surface_area and sphericity serve in 3-D")
    c = p.perimeter_classes.double()
    return c[:, 0] * _PERIMETER_WEIGHTS[0] + c[:, 1] * _PERIMETER_WEIGHTS[1] + c[:, 2] * _PERIMETER_WEIGHTS[2]


def circularity(p: ShapeProps) -> torch.Tensor:
    """``4 pi area / perimeter^2`` with scikit-image's perimeter estimator (2-D only): near 1 for a disk, ``inf`` / NaN where the perimeter is 0."""
    _shape_props(p, "circularity")
    return 4 * math.pi * p.area.double() / perimeter(p) ** 2


def sphericity(p: ShapeProps, sampling=None) -> torch.Tensor:
    """``pi^(1/3) (6 V)^(2/3) / surface_area`` with ``V = area * prod(sampling)``.  Product-defined, NOT the reference's number from a meshed
    surface: as the voxel-face count of a ball tends to 1.5 x its true surface, this tends to 2 / 3 for a ball (and is 0.806 for a cube)."""
    if _shape_props(p, "sphericity") != 3:
        raise ValueError("biapy_amd.prepost.sphericity is defined for 3-D labels only; circularity serves in 2-D")
    v = p.area.double() * math.prod(_sampling(sampling, 3, "sphericity"))
    return math.pi ** (1.0 / 3.0) * (6 * v) ** (2.0 / 3.0) / surface_area(p, sampling)


# ---- morphology: erosion, dilation, boundaries, hole filling and border clearing (csrc/morph.hip) -------------------------------------------------
# The steps BETWEEN the calls above in the instance and detection workflows: seed maps are eroded before label(), holes in the foreground are
# filled, instances that touch the border are dropped, instance targets get their contour channel from find_boundaries, masks are opened or
# closed to remove speckle (scipy.ndimage.binary_* / grey_*, skimage.segmentation.find_boundaries / clear_border on the host there).
# ``connectivity`` is always an int with label()'s meaning: the element is scipy.ndimage.generate_binary_structure(ndim, connectivity).
# NOT offered: arbitrary ``structure`` / ``footprint`` arrays; ``mask=`` and ``origin=``; ``iterations < 1`` (SciPy's "until stable" needs a
# read-back); grey ``mode="constant"`` (out-of-volume neighbours are ignored: SciPy's default "reflect" for these elements); ball footprints on
# grey input; find_boundaries' "outer" / "subpixel"; clear_border's ``buffer_size`` and ``mask``; volumes of 2^31 voxels or
# more; multi-GPU slabs; the watershed_by_channels threshold logic itself, which is now a short sequence of these calls.

_MORPH_ERODE, _MORPH_DILATE, _MORPH_BOUNDARY = 0, 1, 2            # include/biapy_amd.h: bpx_morph's op
_MORPH_BINARY, _MORPH_ABSORB, _MORPH_INNER = 1, 2, 4               # and its flags
_MORPH_DT = {torch.uint8: L.U8, torch.int32: L.I32, torch.float32: L.F32}


def _morph_input(x: torch.Tensor, what: str, dtypes, names: str) -> Tuple[int, int, int]:
    if x.dtype not in dtypes:
        raise NotImplementedError(f"biapy_amd.prepost.{what} works on {names} tensors (got {x.dtype})")
    Z, Y, X = _label_volume(x, what)
    if x.numel() < 1:
        raise NotImplementedError(f"biapy_amd.prepost.{what}: a {tuple(x.shape)} volume has an empty axis")
    return Z, Y, X


def _on_device(x: torch.Tensor) -> torch.Tensor:
    """The last refusal, after every argument has been checked."""
    if not x.is_cuda:
        raise RuntimeError("biapy_amd.prepost runs on the MI355X only (tensor is on %s); there is no CPU path" % x.device)
    return x


def _connectivity(x: torch.Tensor, connectivity) -> int:
    c = int(connectivity)
    if not 1 <= c <= x.dim():
        raise ValueError(f"connectivity must be in 1..{x.dim()} for a {x.dim()}-D tensor (got {connectivity})")
    return c


def _morph(src: torch.Tensor, dst: torch.Tensor, shape, ndim: int, c: int, op: int, flags: int = 0, background: int = 0) -> torch.Tensor:
    """One launch of ``bpx_morph`` from the contiguous ``src`` into ``dst``."""
    Z, Y, X = shape
    L.check(lib.bpx_morph(src.data_ptr(), _MORPH_DT[src.dtype], Z, Y, X, ndim, c, op, flags, int(background), dst.data_ptr(), L.stream_ptr()))
    return dst


def _ball(mask: torch.Tensor, radius, dilate: bool) -> torch.Tensor:
    """Erosion / dilation by the Euclidean ball ``dz^2 + dy^2 + dx^2 <= r^2`` from the exact squared distance transform: a voxel survives the
    erosion when its nearest zero is farther than ``r``, and the dilation reaches it when its nearest one is no farther.  No special case for
    a mask without any zero (erosion) or any one (dilation): the transform then returns its sentinel INT32_MAX, which is "farther than any r",
    so the erosion keeps every voxel and the dilation sets none - the right answers."""
    r2 = min(int(math.floor(float(radius) ** 2)), 2 ** 31 - 2)                 # below the sentinel; no distance in a volume the transform accepts reaches it
    if dilate:
        return (distance_transform_edt(mask == 0, squared=True) <= r2).to(torch.uint8)
    return (distance_transform_edt(mask, squared=True) > r2).to(torch.uint8)


def _binary(mask: torch.Tensor, what: str, dilate: bool, connectivity, iterations, border_value, radius) -> torch.Tensor:
    shape = _morph_input(mask, what, (torch.uint8, torch.bool), "uint8 or bool")
    if border_value not in (0, 1):
        raise ValueError(f"border_value must be 0 or 1 (got {border_value!r})")
    if radius is not None:
        if int(connectivity) != 1 or int(iterations) != 1:
            raise ValueError(f"biapy_amd.prepost.{what}: radius is given INSTEAD of connectivity / iterations (got connectivity={connectivity}, "
                             f"iterations={iterations})")
        if int(border_value) != (0 if dilate else 1):
            raise NotImplementedError(f"biapy_amd.prepost.{what}: radius= is offered with border_value={0 if dilate else 1} only - the other value "
                                      "needs the black border the distance transform does not offer")
        if not (math.isfinite(float(radius)) and float(radius) >= 0.0):
            raise ValueError(f"radius must be a finite number >= 0 (got {radius!r})")
        return _ball(_on_device(mask), radius, dilate)
    c = _connectivity(mask, connectivity)
    k = int(iterations)
    if k < 1:
        raise NotImplementedError(f"biapy_amd.prepost.{what}: iterations must be >= 1 (got {iterations}); SciPy's 'until stable' needs a read-back "
                                  "and is not offered")
    src = _on_device(mask).contiguous()
    if src.dtype == torch.bool:
        src = src.view(torch.uint8)
    absorbing = 1 if dilate else 0
    flags = _MORPH_BINARY | (_MORPH_ABSORB if int(border_value) == absorbing else 0)
    out = torch.empty(mask.shape, dtype=torch.uint8, device=mask.device)
    other = torch.empty_like(out) if k > 1 else None
    for i in range(k):                                             # k launches; the last one writes `out`
        dst = out if (k - 1 - i) % 2 == 0 else other
        src = _morph(src, dst, shape, mask.dim(), c, _MORPH_DILATE if dilate else _MORPH_ERODE, flags)
    return out


def binary_erosion(mask: torch.Tensor, connectivity: int = 1, iterations: int = 1, border_value: int = 0, radius=None) -> torch.Tensor:
    """``scipy.ndimage.binary_erosion(mask, generate_binary_structure(mask.ndim, connectivity), iterations, border_value=border_value)`` of a
    2-D / 3-D ``uint8`` or ``bool`` device mask (every nonzero value is foreground) as a ``uint8`` 0 / 1 mask, bit for bit.  ``iterations = k
    >= 1`` is ``k`` launches that ping-pong between the result and one scratch volume.

    ``radius=r``, given INSTEAD of ``connectivity`` / ``iterations``, erodes by the Euclidean ball ``dz^2 + dy^2 + dx^2 <= r^2`` (scikit-image's
    ``ball(r)`` / ``disk(r)``) by thresholding the exact squared distance transform: ``distance_transform_edt(mask, squared=True) > r^2``.  The
    transform has no black border, so this is offered for ``border_value=1`` only (dilation: ``border_value=0``).

    Nothing is read back, two runs give the same bits, the call can be captured in a graph.  Refused before anything is launched: a CPU tensor
    (``RuntimeError``); other dtypes, an empty axis, 2^31 voxels or more, ``iterations < 1`` (SciPy's "until stable") and ``radius`` with the
    other border value (``NotImplementedError``); other ranks, a connectivity outside ``1..ndim``, a ``border_value`` other than 0 / 1 and
    ``radius`` together with ``connectivity`` / ``iterations`` (``ValueError``).  ``structure``, ``mask`` and ``origin`` are not offered."""
    return _binary(mask, "binary_erosion", False, connectivity, iterations, border_value, radius)


def binary_dilation(mask: torch.Tensor, connectivity: int = 1, iterations: int = 1, border_value: int = 0, radius=None) -> torch.Tensor:
    """``scipy.ndimage.binary_dilation`` with the parameters, the result and the refusals of ``binary_erosion``.  ``radius=r`` is
    ``distance_transform_edt(mask == 0, squared=True) <= r^2`` and is offered for ``border_value=0`` only."""
    return _binary(mask, "binary_dilation", True, connectivity, iterations, border_value, radius)


def binary_opening(mask: torch.Tensor, connectivity: int = 1, iterations: int = 1, border_value: int = 0) -> torch.Tensor:
    """``scipy.ndimage.binary_opening``: the erosion, then the dilation of its result, both with the same ``iterations`` and ``border_value`` -
    the composition SciPy makes, bit for bit.  Removes foreground speckle smaller than the element."""
    return binary_dilation(binary_erosion(mask, connectivity, iterations, border_value), connectivity, iterations, border_value)


def binary_closing(mask: torch.Tensor, connectivity: int = 1, iterations: int = 1, border_value: int = 0) -> torch.Tensor:
    """``scipy.ndimage.binary_closing``: the dilation, then the erosion of its result, both with the same ``iterations`` and ``border_value``.
    Closes gaps smaller than the element."""
    return binary_erosion(binary_dilation(mask, connectivity, iterations, border_value), connectivity, iterations, border_value)


def _grey(x: torch.Tensor, what: str, connectivity, op: int) -> torch.Tensor:
    shape = _morph_input(x, what, (torch.uint8, torch.int32, torch.float32), "uint8, int32 or float32")
    c = _connectivity(x, connectivity)
    return _morph(_on_device(x).contiguous(), torch.empty(x.shape, dtype=x.dtype, device=x.device), shape, x.dim(), c, op)


def erosion(x: torch.Tensor, connectivity: int = 1) -> torch.Tensor:
    """``scipy.ndimage.grey_erosion(x, footprint=generate_binary_structure(x.ndim, connectivity))`` (``skimage.morphology.erosion``) of a 2-D /
    3-D ``uint8``, ``int32`` or ``float32`` device tensor: the minimum over the element, in the input's type; out-of-volume neighbours are
    ignored (SciPy's default ``mode="reflect"`` for these elements).  ``float32``: equal as values - which of ``-0.0`` / ``+0.0`` is chosen is
    unspecified, and so is NaN.  One launch, capturable; the refusals of ``binary_erosion``."""
    return _grey(x, "erosion", connectivity, _MORPH_ERODE)


def dilation(x: torch.Tensor, connectivity: int = 1) -> torch.Tensor:
    """``scipy.ndimage.grey_dilation(x, footprint=generate_binary_structure(x.ndim, connectivity))``: the maximum over the element, otherwise as
    ``erosion``.  On an ``int32`` label volume this is "THE LARGEST NEIGHBOURING ID WINS": a background voxel next to labels 3 and 7 becomes 7,
    and so does a voxel of label 3 next to label 7 - labels grow into the background AND into smaller ids."""
    return _grey(x, "dilation", connectivity, _MORPH_DILATE)


def find_boundaries(labels: torch.Tensor, connectivity: int = 1, mode: str = "thick", background: int = 0) -> torch.Tensor:
    """The boundary map of a 2-D / 3-D label tensor (``int32``; ``uint8`` / ``bool`` and ``float32`` are taken too) as ``uint8`` 0 / 1, in one
    pass: ``mode="thick"`` is ``dilation(labels, connectivity) != erosion(labels, connectivity)`` - a voxel whose element holds two different
    values; ``mode="inner"`` is that AND ``labels != background``, the boundary voxels that belong to an object.  The call shape of
    ``skimage.segmentation.find_boundaries``; the definition is this product's, stated here and checked against its own statement.  ``"outer"``
    and ``"subpixel"`` raise ``NotImplementedError``.  Negative labels are ordinary values.  One launch, capturable."""
    if mode not in ("thick", "inner", "outer", "subpixel"):
        raise ValueError(f"mode must be 'thick' or 'inner' (got {mode!r})")
    if mode in ("outer", "subpixel"):
        raise NotImplementedError(f"biapy_amd.prepost.find_boundaries offers the modes 'thick' and 'inner' (got {mode!r})")
    shape = _morph_input(labels, "find_boundaries", (torch.int32, torch.uint8, torch.bool, torch.float32), "int32, uint8, bool or float32")
    c = _connectivity(labels, connectivity)
    bg = int(background)
    if not -2 ** 31 <= bg < 2 ** 31:
        raise ValueError(f"background must fit int32 (got {background})")
    src = _on_device(labels).contiguous()
    if src.dtype == torch.bool:
        src = src.view(torch.uint8)
    out = torch.empty(labels.shape, dtype=torch.uint8, device=labels.device)
    return _morph(src, out, shape, labels.dim(), c, _MORPH_BOUNDARY, _MORPH_INNER if mode == "inner" else 0, bg)


def _num_labels(lab: torch.Tensor, num) -> int:
    n_max = max(int(lab.max()), 0) if num is None else int(num)
    if n_max < 0:
        raise ValueError(f"num must not be negative (got {n_max})")
    return n_max


def _border_labels(lab: torch.Tensor, n_max: int) -> torch.Tensor:
    """A ``bool`` tensor of length ``n_max + 1``: entry ``l`` is true when a voxel on one of the volume's six faces (four edges in 2-D) carries
    label ``l``.  Torch indexing over the faces only; labels outside ``1..n_max`` land on entry 0, which nobody reads.  Capturable."""
    flags = torch.zeros(n_max + 1, dtype=torch.uint8, device=lab.device)
    for axis in range(lab.dim()):
        for side in (0, lab.shape[axis] - 1):
            face = lab.select(axis, side).reshape(-1).long()
            flags.index_fill_(0, torch.where((face > 0) & (face <= n_max), face, torch.zeros_like(face)), 1)
    return flags != 0


def clear_border(labels: torch.Tensor, num=None, relabel: bool = False, return_num: bool = False):
    """``skimage.segmentation.clear_border(labels)`` on a 2-D / 3-D ``int32`` label tensor: a NEW tensor in which every label that has a voxel on
    the volume's border is 0.  The survivors keep their ids; ``relabel=True`` renumbers them ``1..N'`` in the same order, ``return_num`` adds
    ``N'`` as a 0-d ``int32`` device tensor - ``select_objects`` on the flags of the faces.  ``num`` as in ``region_props``: the largest label as
    a Python int (inside a graph an upper bound serves), the 0-d tensor of ``label``, or ``None``, which reads ``labels.max()`` back; labels above
    it become 0.  ``buffer_size`` and ``mask`` are not offered."""
    n_max = None if num is None else _num_labels(labels, num)
    _label_volume(labels, "clear_border")
    lab = _labels(labels, "clear_border")
    if n_max is None:
        n_max = _num_labels(lab, None)
    return select_objects(lab, ~_border_labels(lab, n_max), relabel=relabel, return_num=return_num)


def binary_fill_holes(mask: torch.Tensor, num=None) -> torch.Tensor:
    """``scipy.ndimage.binary_fill_holes(mask)`` of a 2-D / 3-D ``uint8`` or ``bool`` device mask as a ``uint8`` 0 / 1 mask, bit for bit: the
    background is labelled at connectivity 1 (``label(mask == 0, 1)``), its components that touch no face of the volume are the holes
    (``select_objects``), and they are OR-ed into the mask.  A hole open to the border through one voxel is no hole; one open only through a
    diagonal is.  ``num``: the number of background components - ``None`` reads that one scalar back; an int is an upper bound of it that
    makes the call capturable (components numbered above it would stay unfilled); a 0-d tensor is read back."""
    _morph_input(mask, "binary_fill_holes", (torch.uint8, torch.bool), "uint8 or bool")
    if num is not None and int(num) < 0:
        raise ValueError(f"num must not be negative (got {int(num)})")
    fg = _on_device(mask) != 0
    lab, n = label(~fg, connectivity=1, return_num=True)
    n_max = int(n) if num is None else int(num)
    holes = select_objects(lab, ~_border_labels(lab, n_max))
    return ((holes > 0) | fg).to(torch.uint8)


# ---- local maxima: the detection workflow's points and the watershed's markers (csrc/peaks.hip) ----------------------------------------------------
# The reference's default point-creation function is skimage.feature.peak_local_max(prob, min_distance, threshold_abs, exclude_border) on the
# probability map, and the same call on the distance map gives the markers watershed() needs; both ran on the host.  A local-maximum filter
# with a radius and a deterministic tie rule (the raster-first voxel of equal values wins), a 0 / 1 volume for label() and a compact, sorted
# point list that is never read back.  NOT offered: ``threshold_rel``, ``labels=``, ``footprint=`` and ``p_norm`` (the distance is the box's:
# Chebyshev, per axis); ``blob_log``; the reference's remove_close_points and its point-matching detection metric (host work on kilobytes);
# volumes of 2^31 voxels or more; multi-GPU slabs.

_PEAKS_MAX_RADIUS = 64                                                # csrc/peaks_core.h: PEAKS_MAX_RADIUS


def _per_axis(value, ndim: int, name: str) -> Tuple[int, ...]:
    if isinstance(value, (tuple, list)):
        if len(value) != ndim:
            raise ValueError(f"{name} must be an int or one int per axis of the {ndim}-D image (got {len(value)} values)")
        return tuple(int(v) for v in value)
    return (int(value),) * ndim


def _peaks_call(image: torch.Tensor, what: str, min_distance, threshold_abs, exclude_border, sizes=()):
    """The checks both calls share, in the house order, then the volume, the radii, the margins and the threshold as ``bpx_peak_local_max`` takes
    them.  ``sizes``: ``(name, value)`` pairs that must be ``None`` or at least 1."""
    if image.dim() not in (2, 3):
        raise ValueError(f"biapy_amd.prepost.{what} takes a 2-D (Y, X) or 3-D (Z, Y, X) tensor (got {image.dim()} dimensions)")
    nd = image.dim()
    radii = _per_axis(min_distance, nd, "min_distance")
    if any(r < 0 or r > _PEAKS_MAX_RADIUS for r in radii):
        raise ValueError(f"min_distance must be in 0..{_PEAKS_MAX_RADIUS} on every axis (got {min_distance!r})")
    if exclude_border is True:
        border = radii
    elif exclude_border is False:
        border = (0,) * nd
    else:
        border = _per_axis(exclude_border, nd, "exclude_border")
    if any(b < 0 for b in border):
        raise ValueError(f"exclude_border must not be negative (got {exclude_border!r})")
    for name, v in sizes:
        if v is not None and int(v) < 1:
            raise ValueError(f"{name} must be at least 1 (got {v})")
    if threshold_abs is not None and math.isnan(float(threshold_abs)):
        raise ValueError("threshold_abs must not be NaN")
    if image.dtype not in (torch.float32, torch.int32):
        raise NotImplementedError(f"biapy_amd.prepost.{what} works on float32 or int32 images (got {image.dtype})")
    if image.numel() < 1:
        raise NotImplementedError(f"biapy_amd.prepost.{what}: a {tuple(image.shape)} volume has an empty axis")
    if image.numel() >= 2 ** 31:
        raise NotImplementedError(f"biapy_amd.prepost.{what}: {image.numel()} voxels - volumes of 2^31 voxels or more are not supported (int32 indices)")
    img = _on_device(image).contiguous()
    if threshold_abs is None:                                          # skimage: image.min(); one scalar read back - not capturable
        thr = minmax(img)[0] if img.dtype == torch.float32 else float(int(img.min()))
        if math.isnan(thr):
            raise ValueError(f"biapy_amd.prepost.{what}: the image holds NaN, so threshold_abs=None (the image's minimum) is NaN; pass a threshold")
    else:
        thr = float(threshold_abs)
    pad = (0,) * (3 - nd)
    return img, (1,) * (3 - nd) + tuple(image.shape), pad + radii, pad + border, thr


def _peaks_run(img: torch.Tensor, shape, radii, border, thr: float, mask: Optional[torch.Tensor], keys: Optional[torch.Tensor]) -> torch.Tensor:
    """``bpx_peak_local_max`` into ``mask`` and / or ``keys``; returns the number of peaks (0-d ``int32``, counted past ``keys``' end as well)."""
    Z, Y, X = shape
    need = int(lib.bpx_peaks_workspace(Z, Y, X))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=img.device)
    count = torch.empty((), dtype=torch.int32, device=img.device)
    L.check(lib.bpx_peak_local_max(img.data_ptr(), L.F32 if img.dtype == torch.float32 else L.I32, Z, Y, X, radii[0], radii[1], radii[2], thr,
                                   border[0], border[1], border[2], L.ptr(mask), L.ptr(keys), 0 if keys is None else keys.numel(), count.data_ptr(),
                                   ws.data_ptr(), need, L.stream_ptr()))
    return count


def peak_mask(image: torch.Tensor, min_distance=1, threshold_abs=None, exclude_border=True) -> torch.Tensor:
    """The peaks of ``peak_local_max`` (same parameters, same definition) as a ``uint8`` 0 / 1 tensor of ``image``'s shape - what
    ``skimage.feature.peak_local_max`` returned with ``indices=False``.  ``label(peak_mask(edt, d))`` are the markers of ``watershed``: every
    peak is alone in its box, so at connectivity 1 and ``min_distance >= 1`` each becomes a marker of its own."""
    img, shape, radii, border, thr = _peaks_call(image, "peak_mask", min_distance, threshold_abs, exclude_border)
    mask = torch.empty(image.shape, dtype=torch.uint8, device=img.device)
    _peaks_run(img, shape, radii, border, thr, mask, None)
    return mask


def peak_local_max(image: torch.Tensor, min_distance=1, threshold_abs=None, exclude_border=True, num_peaks: Optional[int] = None,
                   max_peaks: Optional[int] = None, return_values: bool = False):
    """The local maxima of a 2-D ``(Y, X)`` or 3-D ``(Z, Y, X)`` ``float32`` or ``int32`` device tensor: the call shape of
    ``skimage.feature.peak_local_max(image, min_distance, threshold_abs, exclude_border, num_peaks)``, with semantics of its own, stated exactly
    and checked against a host twin (``tests/peaks_ref.py``).  With the radii ``r = min_distance`` (an int, or one int per axis - this package's
    extension for anisotropic volumes; each in ``0..64``):

    * the KEY of voxel ``v`` is ``(k(v) << 32) | (0xFFFFFFFF - linear_index(v))`` as ``uint64``, ``k`` being ``watershed``'s order-preserving
      ``uint32`` image of the value (``int32``: ``v + 2^31``; ``float32``: the sign-flip map, so ``-0.0 < +0.0``; NaN is unspecified): a larger
      key is a larger value, and among equal values the raster-first voxel;
    * a voxel is a PEAK when its key is the maximum of the keys in the box ``[z-rz, z+rz] x [y-ry, y+ry] x [x-rx, x+rx]`` clipped to the volume,
      its value is ``> threshold_abs`` (compared in ``double``, exact for both dtypes), and it lies at least ``b`` voxels from both faces of
      every axis, ``b`` the ``exclude_border`` margin of that axis - on an axis of extent ``<= 2 b`` no voxel does.

    What follows from that:

    * no two peaks ever lie in each other's box (each key would have to exceed the other), so scikit-image's ``ensure_spacing`` pass has nothing
      left to do and is not made;
    * on an image without two equal values inside any box the peaks are scikit-image's:
      ``(image == maximum_filter(image, size=2r+1, mode="nearest")) & (image > threshold_abs)`` with the border cleared;
    * ON TIES THE PEAKS ARE A SUBSET of that mask: a constant plateau the size of a box yields its raster-first voxel only, where
      scikit-image keeps several spaced points of a long plateau.  A ``1 x 21`` row with a plateau at ``x = 3..14`` and radii ``(0, 2)`` gives
      the one peak ``(0, 3)``; scikit-image's mask holds 12 voxels there.

    ``exclude_border`` follows scikit-image: ``True`` is ``min_distance``, ``False`` is 0, or an int, or one int per axis.  ``threshold_abs=None``
    follows it too and means ``image.min()`` (the voxels that carry the minimum are no peaks): THAT CALL FORM READS ONE SCALAR BACK and cannot
    be captured in a graph; with a given threshold (``-inf`` for none) nothing is read back, two runs give the same bits and the call can be
    captured.  ``threshold_rel``, ``labels``, ``footprint`` and ``p_norm`` are not offered.

    Returns ``(coords, num)``, or ``(coords, values, num)`` with ``return_values``:

    * ``coords``: ``int32`` of shape ``(max_peaks, ndim)``, SORTED by value descending, then by linear index ascending (one ``torch.sort`` of
      the key array, descending); the rows from ``num`` onward are ``-1``;
    * ``values``: ``image``'s dtype, the peaks' values decoded from the keys bit for bit; 0 from ``num`` onward;
    * ``num``: the number of peaks as a 0-d ``int32`` DEVICE tensor, ``-1`` when there are more than ``max_peaks`` of them (the other results
      are then unspecified).

    ``max_peaks`` defaults to ``min(n, 2**20)``.  ``num_peaks=k`` keeps the first ``k`` rows: the results have ``min(k, max_peaks)`` rows and
    ``num`` is ``min(num, k)``.

    One launch that clears the outputs and one pass per axis with a nonzero radius and more than one voxel (one pass when there is none), fixed by the shape and the radii
    (``csrc/peaks.hip``); at most ``2 r + 4`` loads per voxel and axis, never the box.  The workspace is 16 bytes per voxel (two key volumes).

    Refused before anything is launched: other ranks, a ``min_distance`` / ``exclude_border`` tuple of another length, a radius outside
    ``0..64``, a negative margin, ``max_peaks`` / ``num_peaks < 1`` and a NaN threshold (``ValueError``); other dtypes, an empty axis and 2^31
    voxels or more (``NotImplementedError``); last, a CPU tensor (``RuntimeError``)."""
    img, shape, radii, border, thr = _peaks_call(image, "peak_local_max", min_distance, threshold_abs, exclude_border,
                                                 (("max_peaks", max_peaks), ("num_peaks", num_peaks)))
    n = img.numel()
    mp = min(n, 2 ** 20) if max_peaks is None else min(int(max_peaks), 2 ** 31 - 1)
    keys = torch.empty(mp, dtype=torch.int64, device=img.device)       # uint64 bits
    count = _peaks_run(img, shape, radii, border, thr, None, keys)
    top = torch.iinfo(torch.int64).min                                 # bit 63: signed order of key ^ top = unsigned order of key
    keys = torch.sort(keys ^ top, descending=True).values ^ top       # the filler 0 is below every key
    num = torch.where(count > mp, torch.full_like(count, -1), count)
    if num_peaks is not None:
        keys = keys[:int(num_peaks)]
        num = torch.clamp(num, max=int(num_peaks))
    filler = keys == 0
    index = 0xFFFFFFFF - (keys & 0xFFFFFFFF)
    _, Y, X = shape
    zyx = torch.stack((index // (Y * X), index // X % Y, index % X), dim=1)[:, 3 - image.dim():]
    coords = zyx.masked_fill(filler[:, None], -1).to(torch.int32)
    if not return_values:
        return coords, num
    k = (keys >> 32) & 0xFFFFFFFF                                      # the value's order-preserving uint32 image, in int64
    if img.dtype == torch.float32:
        bits = torch.where(k >= 2 ** 31, k - 2 ** 31, 0xFFFFFFFF - k)  # the sign-flip map back
        bits = bits - ((bits >> 31) << 32)                             # the same 32 bits as a signed number
        values = bits.masked_fill(filler, 0).to(torch.int32).view(torch.float32)
    else:
        values = (k - 2 ** 31).masked_fill(filler, 0).to(torch.int32)
    return coords, values, num


# ---- median filter: the first step of the reference's post-processing of a prediction (csrc/median.hip) ---------------------------------------------
# POST_PROCESSING.MEDIAN_FILTER with MEDIAN_FILTER_AXIS / MEDIAN_FILTER_SIZE in the reference's configuration (key names from memory, unverified)
# runs scipy.ndimage.median_filter over the float probability volume on the host before any threshold, with a per-axis size that is 1 on the
# axes not named.  Exact selection on order-preserving keys, so the call is held against SciPy as values and against a NumPy twin bit for bit.
# NOT offered: even sizes (SciPy shifts the window's origin there), sizes above 15, windows of more than 125 voxels, ``footprint=``,
# ``origin=``, ``output=``, the modes "mirror" and "wrap", rank and percentile filters; volumes of 2^31 voxels or more; multi-GPU slabs.

_MEDIAN_MAX_SIZE = 15                                                 # csrc/median_core.h: MEDIAN_MAX_SIZE
_MEDIAN_MAX_WINDOW = 125                                              # csrc/median_core.h: MEDIAN_MAX_WINDOW
_MEDIAN_MODES = {"reflect": 0, "nearest": 1, "constant": 2}           # include/biapy_amd.h: bpx_median_filter's mode
_MEDIAN_AXES = ("xy", "yx", "yz", "zy", "zx", "xz", "z", "y", "x", "xyz")


def _median_sizes(size, ndim: int) -> Tuple[int, ...]:
    sizes = _per_axis(size, ndim, "size")
    if any(s < 1 for s in sizes):
        raise ValueError(f"size must be at least 1 on every axis (got {size!r})")
    if any(s % 2 == 0 for s in sizes):
        raise NotImplementedError(f"biapy_amd.prepost.median_filter: size must be odd on every axis (got {size!r}); SciPy shifts the window's "
                                  "origin for an even size and that is not offered")
    if any(s > _MEDIAN_MAX_SIZE for s in sizes):
        raise NotImplementedError(f"biapy_amd.prepost.median_filter: size must be at most {_MEDIAN_MAX_SIZE} on every axis (got {size!r})")
    if math.prod(sizes) > _MEDIAN_MAX_WINDOW:
        raise NotImplementedError(f"biapy_amd.prepost.median_filter: a window of {math.prod(sizes)} voxels (size {size!r}); at most "
                                  f"{_MEDIAN_MAX_WINDOW} are supported")
    return sizes


def median_filter(x: torch.Tensor, size=3, mode: str = "reflect", cval: float = 0.0) -> torch.Tensor:
    """``scipy.ndimage.median_filter(x, size=size, mode=mode, cval=cval)`` of a 2-D ``(Y, X)`` or 3-D ``(Z, Y, X)`` device tensor, as a tensor of
    ``x``'s shape and dtype: ``float32`` (probabilities, distance maps), ``uint8`` (masks, class maps) or ``bool`` (viewed as ``uint8``, ``bool``
    comes back: the median of a binary mask is the majority vote).  Channels are the caller's loop: ``x[..., c]``; a non-contiguous view is made
    contiguous.

    ``size`` is an int or one int per axis in ``(z, y, x)`` order, every entry odd and in ``1..15``, the window ``W = sz * sy * sx <= 125``
    voxels; ``W = 1`` returns a copy.  ``mode`` is ``"reflect"`` (SciPy's default, ``d c b a | a b c d``, over as many periods as the window
    needs), ``"nearest"`` or ``"constant"`` with ``cval`` (finite for ``float32``, an integer in ``0..255`` for ``uint8`` / ``bool``).

    The result at a voxel is the element of rank ``W // 2`` among the ``W`` window values, ordered by their order-preserving ``uint32`` key -
    ``float32``: ``bits | 0x80000000`` for a clear sign bit, ``~bits`` otherwise; ``uint8``: the value - and returned with its bits.  That is
    SciPy's result as values, and the NumPy twin ``tests/median_ref.py`` bit for bit.  Two points SciPy leaves open are stated: ``-0.0`` sorts
    below ``+0.0``, and NaNs sort by their bits (negative-sign NaNs below ``-inf``, positive-sign NaNs above ``+inf`` - product-defined).
    Nothing is computed, so nothing is flushed: denormals come back as they went in.

    One launch (``csrc/median.hip``): a block stages its tile and halo into LDS as keys and every thread selects in registers.  No workspace,
    nothing read back, two runs give the same bits, the call can be captured in a graph.

    Refused before anything is launched, in this order: other dtypes (``NotImplementedError``), other ranks (``ValueError``), an empty axis
    (``NotImplementedError``); a ``size`` of another length or below 1 (``ValueError``), even, above 15 or with ``W > 125``
    (``NotImplementedError``); ``"mirror"`` / ``"wrap"`` (``NotImplementedError``) and unknown modes (``ValueError``); a ``cval`` the dtype
    cannot hold (``ValueError``); 2^31 voxels or more (``NotImplementedError``); last, a CPU tensor (``RuntimeError``).  ``footprint``,
    ``origin`` and ``output`` are not offered."""
    sizes, m, c = _median_check(x, size, mode, cval)
    return _median_run(_on_device(x), sizes, m, c)


def _median_check(x: torch.Tensor, size, mode, cval):
    """Every refusal of ``median_filter`` but the last, in the house order; the sizes, the mode's code and ``cval`` as ``bpx_median_filter`` takes them."""
    what = "median_filter"
    if x.dtype not in (torch.float32, torch.uint8, torch.bool):
        raise NotImplementedError(f"biapy_amd.prepost.{what} works on float32, uint8 or bool tensors (got {x.dtype})")
    if x.dim() not in (2, 3):
        raise ValueError(f"biapy_amd.prepost.{what} takes a 2-D (Y, X) or 3-D (Z, Y, X) tensor (got {x.dim()} dimensions)")
    if x.numel() < 1:
        raise NotImplementedError(f"biapy_amd.prepost.{what}: a {tuple(x.shape)} volume has an empty axis")
    sizes = _median_sizes(size, x.dim())
    if mode in ("mirror", "wrap"):
        raise NotImplementedError(f"biapy_amd.prepost.{what}: mode {mode!r} is not offered (reflect, nearest or constant)")
    if mode not in _MEDIAN_MODES:
        raise ValueError(f"mode must be 'reflect', 'nearest' or 'constant' (got {mode!r})")
    c = float(cval)
    if x.dtype == torch.float32:
        if not (math.isfinite(c) and abs(c) <= 3.4028234663852886e38):
            raise ValueError(f"cval must be finite as float32 (got {cval!r})")
    elif not (math.isfinite(c) and c == math.floor(c) and 0.0 <= c <= 255.0):
        raise ValueError(f"cval must be an integer in 0..255 for a {x.dtype} tensor (got {cval!r})")
    if x.numel() >= 2 ** 31:
        raise NotImplementedError(f"biapy_amd.prepost.{what}: {x.numel()} voxels - volumes of 2^31 voxels or more are not supported (int32 indices)")
    return sizes, _MEDIAN_MODES[mode], c


def _median_run(x: torch.Tensor, sizes, mode: int, cval: float) -> torch.Tensor:
    """One launch of ``bpx_median_filter`` on the checked device tensor ``x``."""
    src = x.contiguous()
    if src.dtype == torch.bool:
        src = src.view(torch.uint8)
    out = torch.empty(x.shape, dtype=src.dtype, device=src.device)
    Z, Y, X = (1,) * (3 - x.dim()) + tuple(x.shape)
    sz, sy, sx = (1,) * (3 - x.dim()) + tuple(sizes)
    L.check(lib.bpx_median_filter(src.data_ptr(), L.F32 if src.dtype == torch.float32 else L.U8, Z, Y, X, sz, sy, sx, mode, cval, out.data_ptr(),
                                  L.stream_ptr()))
    return out.view(torch.bool) if x.dtype == torch.bool else out


def median_filter_axes(x: torch.Tensor, axes, size) -> torch.Tensor:
    """The reference's call shape on one 3-D ``(Z, Y, X)`` channel: ``median_filter`` with ``size`` along the axes that ``axes`` names and 1
    along the others, ``mode="reflect"``.  ``axes`` is one of ``'xy' 'yx' 'yz' 'zy' 'zx' 'xz' 'z' 'y' 'x' 'xyz'`` with an int ``size``, or a list
    of them with a list of one size each, applied in sequence as the reference's loop does (each step filters the result of the one before).
    ``median_filter_axes(p, 'xy', 5)`` is ``median_filter(p, (1, 5, 5))``.  No kernel of its own; the refusals are ``median_filter``'s, after a
    ``ValueError`` for an ``axes`` that is none of the above, lists of different lengths, or a tensor that is not 3-D."""
    if isinstance(axes, str):
        axes, size = [axes], [size]
    elif not isinstance(size, (tuple, list)) or len(size) != len(axes):
        raise ValueError(f"a list of axes takes a list of one size each (got axes {axes!r}, size {size!r})")
    for a in axes:
        if a not in _MEDIAN_AXES:
            raise ValueError(f"axes must be one of {', '.join(repr(v) for v in _MEDIAN_AXES)} (got {a!r})")
    if x.dtype in (torch.float32, torch.uint8, torch.bool) and x.dim() != 3:
        raise ValueError(f"biapy_amd.prepost.median_filter_axes takes a 3-D (Z, Y, X) tensor (got {x.dim()} dimensions)")
    steps = [_median_check(x, tuple(int(s) if ax in a else 1 for ax in "zyx"), "reflect", 0.0) for a, s in zip(axes, size)]
    x = _on_device(x)
    for sizes, m, c in steps:                                          # every step is checked before the first one is launched
        x = _median_run(x, sizes, m, c)
    return x


# ---- separable filter: linear smoothing of an image or a probability map (csrc/sepfilter.hip) --------------------------------------------------------
# DATA.PREPROCESS.GAUSSIAN_BLUR in the reference's configuration (key name from memory, unverified) calls skimage.filters.gaussian, which is
# scipy.ndimage.gaussian_filter per channel; the detection workflow smooths the probability map before peak_local_max, and blob_log starts from
# gaussian_laplace.  One separable correlation with run-time per-axis weights serves all three; the Gaussian is one way to fill the weights.
# NOT offered: uint8 / integer input, ``output=``, ``axes=``, mode "wrap", radii above 32, ``uniform_filter``, ``blob_log``; volumes of 2^31
# voxels or more; multi-GPU slabs.

_SEPFILTER_MAX_RADIUS = 32                                            # csrc/sepfilter_core.h: SEPFILTER_MAX_RADIUS
_SEPFILTER_MODES = {"reflect": 0, "mirror": 1, "nearest": 2, "constant": 3}     # include/biapy_amd.h: bpx_sepfilter's mode


def _sepfilter_input(x: torch.Tensor, what: str) -> None:
    if x.dtype != torch.float32:
        raise NotImplementedError(f"biapy_amd.prepost.{what} works on float32 tensors (got {x.dtype}); call .float() first")
    if x.dim() not in (2, 3):
        raise ValueError(f"biapy_amd.prepost.{what} takes a 2-D (Y, X) or 3-D (Z, Y, X) tensor (got {x.dim()} dimensions)")
    if x.numel() < 1:
        raise NotImplementedError(f"biapy_amd.prepost.{what}: a {tuple(x.shape)} volume has an empty axis")


def _sepfilter_border(x: torch.Tensor, what: str, mode, cval) -> Tuple[int, float]:
    if mode == "wrap":
        raise NotImplementedError(f"biapy_amd.prepost.{what}: mode 'wrap' is not offered (reflect, mirror, nearest or constant)")
    if mode not in _SEPFILTER_MODES:
        raise ValueError(f"mode must be 'reflect', 'mirror', 'nearest' or 'constant' (got {mode!r})")
    c = float(cval)
    if not (math.isfinite(c) and abs(c) <= 3.4028234663852886e38):
        raise ValueError(f"cval must be finite as float32 (got {cval!r})")
    if x.numel() >= 2 ** 31:
        raise NotImplementedError(f"biapy_amd.prepost.{what}: {x.numel()} voxels - volumes of 2^31 voxels or more are not supported (int32 indices)")
    return _SEPFILTER_MODES[mode], c


def _sepfilter_run(x: torch.Tensor, weights, mode: int, cval: float) -> torch.Tensor:
    """``bpx_sepfilter`` on the checked device tensor ``x``: ``weights`` holds one contiguous ``float32`` array or ``None`` per axis of ``x``."""
    src = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.float32, device=src.device)
    Z, Y, X = (1,) * (3 - x.dim()) + tuple(x.shape)
    ws3 = (None,) * (3 - x.dim()) + tuple(weights)
    radii = [-1 if w is None else (len(w) - 1) // 2 for w in ws3]
    need = int(lib.bpx_sepfilter_workspace(Z, Y, X, *radii))
    ws = torch.empty(need // 4, dtype=torch.float32, device=src.device) if need > 0 else None
    wp = [None if w is None else w.ctypes.data for w in ws3]         # host pointers: copied into the kernel arguments before the call returns
    L.check(lib.bpx_sepfilter(src.data_ptr(), Z, Y, X, wp[0], radii[0], wp[1], radii[1], wp[2], radii[2], mode, cval, out.data_ptr(), L.ptr(ws),
                              max(need, 0), L.stream_ptr()))
    return out


def separable_filter(x: torch.Tensor, weights, mode: str = "reflect", cval: float = 0.0) -> torch.Tensor:
    """``scipy.ndimage.correlate1d`` along each given axis in turn, of a 2-D ``(Y, X)`` or 3-D ``(Z, Y, X)`` ``float32`` device tensor, as a new
    ``float32`` tensor.  ``weights`` holds one entry per axis of ``x``, in ``(z, y, x)`` order: ``None`` (the axis is skipped) or a 1-D sequence of
    ``2 r + 1`` floats, ``r`` in ``0..32``, rounded to ``float32``.  Channels are the caller's loop; a non-contiguous view is made contiguous.

    The arithmetic is product-defined: along an axis, ``acc = w[0] * v[f(i - r)]``, then ``acc = acc + w[j] * v[f(i + j - r)]`` for ``j = 1 ..
    2 r`` in that order, every ``*`` and ``+`` one IEEE ``float32`` operation (no FMA, no folded taps, denormals kept); the ``float32`` result of
    one axis is the input of the next, z then y then x.  ``f`` is the border: ``"reflect"`` (``d c b a | a b c d``), ``"mirror"`` (``d c b | a b
    c d``), ``"nearest"`` or ``"constant"`` with ``float32(cval)``, over as many periods as ``r`` needs.  The NumPy twin ``tests/gauss_ref.py``
    gives the same bits; SciPy's ``float64`` result lies within the per-element bound derived there.

    One launch per given axis (``csrc/sepfilter.hip``), the weights by value in the kernel arguments; a workspace of one volume when two or more
    axes are given.  Nothing read back, two runs give the same bits, the call can be captured in a graph.  With no axis given the result is a
    copy.

    Refused before anything is launched, in this order: other dtypes (``NotImplementedError``), other ranks (``ValueError``), an empty axis
    (``NotImplementedError``); ``weights`` of another length, an entry that is not 1-D, of even length or not finite as ``float32``
    (``ValueError``), more than 65 taps (``NotImplementedError``); ``"wrap"`` (``NotImplementedError``) and unknown modes (``ValueError``); a
    ``cval`` that is not finite as ``float32`` (``ValueError``); 2^31 voxels or more (``NotImplementedError``); last, a CPU tensor
    (``RuntimeError``)."""
    what = "separable_filter"
    _sepfilter_input(x, what)
    if not isinstance(weights, (tuple, list)) or len(weights) != x.dim():
        raise ValueError(f"weights must hold one entry (None or a 1-D sequence) per axis of the {x.dim()}-D tensor (got {weights!r})")
    ws = []
    for w in weights:
        if w is None:
            ws.append(None)
            continue
        w64 = np.asarray(w, dtype=np.float64)
        if w64.ndim != 1 or w64.size % 2 == 0:
            raise ValueError(f"every entry of weights must be a 1-D sequence of odd length (got shape {w64.shape})")
        with np.errstate(over="ignore"):
            w32 = np.ascontiguousarray(w64.astype(np.float32))
        if not np.isfinite(w32).all():
            raise ValueError("every weight must be finite as float32")
        ws.append(w32)
    for w in ws:
        if w is not None and w.size > 2 * _SEPFILTER_MAX_RADIUS + 1:
            raise NotImplementedError(f"biapy_amd.prepost.{what}: {w.size} taps on an axis; at most {2 * _SEPFILTER_MAX_RADIUS + 1} "
                                      f"(radius {_SEPFILTER_MAX_RADIUS}) are supported")
    m, c = _sepfilter_border(x, what, mode, cval)
    return _sepfilter_run(_on_device(x), ws, m, c)


def _gaussian_weights(sigma: float, order: int, radius: int) -> np.ndarray:
    """The ``float64`` weights ``scipy.ndimage.gaussian_filter1d`` hands to ``correlate1d``: the sampled Gaussian normalised to sum 1, times the
    polynomial of its ``order``-th derivative, reversed (a correlation, not a convolution).  SciPy's arithmetic restated step by step, so the
    ``float64`` values are the same bits."""
    exponent_range = np.arange(order + 1)
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    phi_x = phi_x / phi_x.sum()
    if order == 0:
        return phi_x[::-1]
    q = np.zeros(order + 1)
    q[0] = 1
    D = np.diag(exponent_range[1:], 1)                                 # D @ q(x) = q'(x)
    P = np.diag(np.ones(order) / -sigma2, -1)                          # P @ q(x) = q(x) * p'(x), p'(x) = -1 / sigma^2
    Q_deriv = D + P
    for _ in range(order):
        q = Q_deriv.dot(q)
    q = (x[:, None] ** exponent_range).dot(q)
    return (q * phi_x)[::-1]


def _per_axis_of(value, ndim: int, name: str) -> list:
    if isinstance(value, (tuple, list)):
        if len(value) != ndim:
            raise ValueError(f"{name} must be a scalar or one value per axis of the {ndim}-D tensor (got {len(value)} values)")
        return list(value)
    return [value] * ndim


def _gaussian_check(x: torch.Tensor, what: str, sigma, order, mode, cval, truncate, radius):
    """Every refusal of ``gaussian_filter`` but the last, in the house order; the ``float32`` weights per axis (``None``: skipped), the mode's code
    and ``cval`` as ``bpx_sepfilter`` takes them."""
    _sepfilter_input(x, what)
    nd = x.dim()
    sigmas = [float(v) for v in _per_axis_of(sigma, nd, "sigma")]
    orders = _per_axis_of(order, nd, "order")
    radii = _per_axis_of(radius, nd, "radius")
    if any(math.isnan(sd) or sd < 0 for sd in sigmas):
        raise ValueError(f"sigma must not be negative (got {sigma!r})")
    if any(isinstance(o, bool) or int(o) != o or not 0 <= int(o) <= 2 for o in orders):
        raise ValueError(f"order must be 0, 1 or 2 on every axis (got {order!r})")
    t = float(truncate)
    if not (math.isfinite(t) and t >= 0):
        raise ValueError(f"truncate must be finite and not negative (got {truncate!r})")
    if any(r is not None and (isinstance(r, bool) or int(r) != r or int(r) < 0) for r in radii):
        raise ValueError(f"radius must be None or a non-negative integer on every axis (got {radius!r})")
    plan = []
    for sd, o, r in zip(sigmas, orders, radii):
        if sd <= 1e-15:                                                # SciPy skips the axis
            plan.append(None)
            continue
        lw = int(t * sd + 0.5) if r is None else int(r)
        if lw > _SEPFILTER_MAX_RADIUS:
            cause = f"sigma {sd:g} with truncate {t:g}" if r is None else f"radius={lw} (sigma {sd:g})"
            raise NotImplementedError(f"biapy_amd.prepost.{what}: {cause} needs a radius of {lw} voxels; at most {_SEPFILTER_MAX_RADIUS} are supported")
        plan.append((sd, int(o), lw))
    m, c = _sepfilter_border(x, what, mode, cval)
    ws = [None if p is None else np.ascontiguousarray(_gaussian_weights(*p).astype(np.float32)) for p in plan]
    return ws, m, c


def gaussian_filter(x: torch.Tensor, sigma, order=0, mode: str = "reflect", cval: float = 0.0, truncate: float = 4.0, radius=None) -> torch.Tensor:
    """``scipy.ndimage.gaussian_filter(x, sigma, order=order, mode=mode, cval=cval, truncate=truncate, radius=radius)`` of a 2-D ``(Y, X)`` or 3-D
    ``(Z, Y, X)`` ``float32`` device tensor, as a new ``float32`` tensor.  ``sigma``, ``order`` (0, 1 or 2: the Gaussian, its first or second
    derivative) and ``radius`` are a scalar or one value per axis in ``(z, y, x)`` order; an axis with ``sigma <= 1e-15`` is skipped, as SciPy
    does; the radius of an axis is ``int(truncate * sigma + 0.5)`` unless given, at most 32.  Channels are the caller's loop; a non-contiguous view
    is made contiguous.

    The weights are SciPy's, computed in NumPy ``float64`` on the host with SciPy's own steps and then rounded to ``float32``; the filtering is
    ``separable_filter``'s stated ``float32`` arithmetic (product-defined: one multiply and one add per tap in tap order, no FMA, denormals
    kept, z then y then x).  The NumPy twin ``tests/gauss_ref.py`` gives the same bits; ``scipy.ndimage.gaussian_filter`` of the ``float64``
    image lies within the per-element bound derived there.

    One launch per filtered axis (``csrc/sepfilter.hip``), nothing read back, two runs give the same bits, the call can be captured in a graph.

    Refused before anything is launched, in this order: other dtypes (``NotImplementedError``, call ``.float()``), other ranks
    (``ValueError``), an empty axis (``NotImplementedError``); ``sigma`` / ``order`` / ``radius`` of another length, a negative sigma, an order
    outside 0..2, a negative truncate or radius (``ValueError``); a radius above 32 (``NotImplementedError``, naming the sigma); ``"wrap"``
    (``NotImplementedError``) and unknown modes (``ValueError``); a ``cval`` that is not finite as ``float32`` (``ValueError``); 2^31 voxels or
    more (``NotImplementedError``); last, a CPU tensor (``RuntimeError``).  ``output`` and ``axes`` are not offered."""
    ws, m, c = _gaussian_check(x, "gaussian_filter", sigma, order, mode, cval, truncate, radius)
    return _sepfilter_run(_on_device(x), ws, m, c)


def gaussian_laplace(x: torch.Tensor, sigma, mode: str = "reflect", cval: float = 0.0, truncate: float = 4.0) -> torch.Tensor:
    """``scipy.ndimage.gaussian_laplace(x, sigma, mode=mode, cval=cval, truncate=truncate)``: the sum over the axes of ``gaussian_filter`` with
    ``order = 2`` on that axis and 0 on the others - the scale-space operator of ``blob_log`` (``blob_log`` itself is not offered).  The
    ``float32`` adds run in axis order z, y, x as torch adds on the device; each term is ``gaussian_filter``'s stated arithmetic, so the twin of
    ``tests/gauss_ref.py`` gives the same bits.  Two (2-D) or three (3-D) ``gaussian_filter`` calls and one add each after the first; the
    refusals are ``gaussian_filter``'s, every term checked before the first is launched."""
    what = "gaussian_laplace"
    _sepfilter_input(x, what)
    nd = x.dim()
    terms = [_gaussian_check(x, what, sigma, [2 if a == axis else 0 for a in range(nd)], mode, cval, truncate, None) for axis in range(nd)]
    x = _on_device(x)
    out = None
    for ws, m, c in terms:
        g = _sepfilter_run(x, ws, m, c)
        out = g if out is None else out.add_(g)
    return out
