"""MI355X-native Social Force Model stepper behind the reference's PedestrianSimulation / Force API.

Hot path only: forces.py + stateutils.py + the numeric half of
pedestrian_simulation.py of felixlutz/carla-social-force-model, as hand-written HIP kernels for gfx950
called through the C ABI in ``include/sfm_hip.h``.  Import as ``carla_social_force_model_amd``.
"""
__version__ = "0.1.0"


def __getattr__(name):
    # batched scenes (batch.py), imported on first use so that importing the package stays light
    if name in ("SfmBatch", "pack_scenes", "pack_boxes", "split_frames"):
        from . import batch
        return getattr(batch, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
