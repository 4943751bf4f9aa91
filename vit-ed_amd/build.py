"""``build_model(config)`` - the reference's model factory (models/build.py:15-95), pjs branch.

Reads exactly the keys the reference reads for ``MODEL.TYPE == 'pjs'`` (models/build.py:19-32) and
returns the HIP-backed module.  The other model types (timm ViT, SimSiam, ResNet baselines) are not
part of the ViT-ED hot path and are rejected with a clear message.
"""
from .model import VisionTransformerCustom


def build_model(config, is_pretrain=False, drop_path_rate=None, qk_norm=None, patch_drop_rate=None, global_pool='token', fc_norm=None,
                pos_drop_rate=None):
    """``drop_path_rate``: stochastic depth.  The default (None) reads exactly the keys the reference reads, and the reference's
    factory does not forward ``MODEL.DROP_PATH_RATE`` to the pjs model - the shipped YAMLs set it to 0.1 without effect.  Pass
    ``drop_path_rate=config.MODEL.DROP_PATH_RATE`` to train the regularised model those configs describe.
    ``qk_norm``: q/k-norm in every attention.  The reference's factory has no config key for it, so the default (None) leaves it off;
    ``qk_norm=True`` builds the model with ``q_norm`` / ``k_norm`` (a checkpoint of the reference class trained with it loads).
    ``patch_drop_rate``: timm PatchDropout in training mode, which the reference's class inherits and its factory has no key for
    either; the default (None) leaves it off.
    ``global_pool`` / ``fc_norm``: timm's head options ('token' | 'avg'; None | bool), inherited by the reference's class and without a
    config key too; the defaults are the reference's own and build the shipped model.
    ``pos_drop_rate``: timm's dropout behind the position embedding, training mode only; the reference's factory has no key for it
    either, and the default (None) leaves it off."""
    model_type = config.MODEL.TYPE
    if model_type != 'pjs':
        raise NotImplementedError(
            f"MODEL.TYPE={model_type!r}: only the 'pjs' ViT encoder-decoder is implemented on MI355X "
            f"(the other families are baselines outside the accelerated path)")
    pjs = config.MODEL.PJS
    return VisionTransformerCustom(
        img_size=config.DATA.IMG_SIZE,
        patch_size=pjs.PATCH_SIZE,
        in_chans=pjs.IN_CHANS,
        num_classes=config.MODEL.NUM_CLASSES,
        embed_dim=pjs.EMBED_DIM,
        depth=pjs.DEPTH,
        c_depth=pjs.C_DEPTH,
        num_heads=pjs.NUM_HEADS,
        mlp_ratio=pjs.MLP_RATIO,
        qkv_bias=pjs.QKV_BIAS,
        keep_attn=pjs.KEEP_ATTN,
        arch_version=pjs.ARCH_VERSION,
        drop_path_rate=0. if drop_path_rate is None else drop_path_rate,
        qk_norm=bool(qk_norm),
        patch_drop_rate=0. if patch_drop_rate is None else patch_drop_rate,
        global_pool=global_pool,
        fc_norm=fc_norm,
        pos_drop_rate=0. if pos_drop_rate is None else pos_drop_rate,
    )
