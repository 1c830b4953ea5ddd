"""biapy_amd - MI355X (gfx950) native 3D patch U-Net hot path for BiaPy.

Public surface mirrors the reference names for this path:
  biapy_amd.resunet.ResUNet                       <- biapy.models.resunet.ResUNet
  biapy_amd.unet.U_Net                            <- biapy.models.unet.U_Net (2D and 3D)
  biapy_amd.rcan.rcan                             <- biapy.models.rcan.rcan (3D trunk, upscaling_layer=False)
  biapy_amd.tiling.crop_3D_data_with_overlap      <- biapy.data.data_3D_manipulation.crop_3D_data_with_overlap
  biapy_amd.tiling.merge_3D_data_with_overlap     <- biapy.data.data_3D_manipulation.merge_3D_data_with_overlap
  biapy_amd.workflow.SlidingWindowPredictor       <- Base_Workflow.process_test_sample (per-patch branch)
  biapy_amd.chunked.ChunkedPredictor / ChunkGrid  <- chunked_test_pair_data_generator + process_test_sample_by_chunks (in-HBM volumes)
  biapy_amd.train_engine.train_one_epoch/evaluate <- biapy.engine.train_engine.train_one_epoch / evaluate
  biapy_amd.augment.DeviceAugmenter               <- the flips / rot90 / brightness / contrast / noise / cutout subset of biapy.data.generators.augmentors
  biapy_amd.sampler.DevicePatchSampler / DevicePatchLoader <- random patch extraction (DATA.EXTRACT_RANDOM_PATCH, probability map) from resident volumes
  biapy_amd.n2v.N2VMasker (also biapy_amd.N2VMasker) + losses.N2VLoss <- the Noise2Void blind-spot manipulation of the denoising generator and n2v_loss_mse
  biapy_amd.targets.InstanceTargets (also biapy_amd.InstanceTargets) + prepost.instance_targets <- the instance-segmentation channel targets (F, C, D, Dc, H, V, Z) from id patches, on the device
  biapy_amd.losses / prepost / tta               <- biapy.engine.metrics, biapy.data.norm + semantic_seg Otsu, biapy.data.post_processing TTA
"""
__version__ = "0.1.0"


def __getattr__(name):
    # N2VMasker and InstanceTargets load the HIP library on first use, as every other module of the package does on its own import
    if name == "N2VMasker":
        from .n2v import N2VMasker

        return N2VMasker
    if name == "InstanceTargets":
        from .targets import InstanceTargets

        return InstanceTargets
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
