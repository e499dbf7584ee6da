"""clipmi — MI355X-native CLIP dual-encoder + adapter contrastive fine-tuning path.

Drop-in mirrors of the reference's ``model_m.CLIPWithAdapters`` and
``trainer.CLIPAdapterTrainer`` whose compute runs on libclipmi (hand-written HIP for
gfx950, C ABI in include/clipmi.h)."""
from .config import CLIPConfig, PRESETS, TowerConfig, resolve  # noqa: F401


def __getattr__(name):
    # torch-dependent pieces load lazily so config/synth stay importable without a GPU stack
    if name == "CLIPWithAdapters":
        from .model import CLIPWithAdapters
        return CLIPWithAdapters
    if name == "CLIPTokenizer":  # caption BPE of the input step (dataset.py:152-159)
        from .tokenizer import CLIPTokenizer
        return CLIPTokenizer
    if name in ("ContextAdapter", "SharedAdapter", "TextualAdapter"):  # adapter/peclip.py's modules
        from . import peclip
        return getattr(peclip, name)
    if name in ("CLIPAdapterTrainer", "FusedAdamW"):
        from . import trainer
        return getattr(trainer, name)
    if name in _IMAGES:  # ragged image batches and augmentation on the GPU input step
        from . import images
        return getattr(images, name)
    if name in _EVALUATION:  # on-device retrieval ranks and classification metrics
        from . import evaluation
        return getattr(evaluation, name)
    if name in _HEADS:  # the multi-label (sigmoid / BCE) feature-level head
        from . import heads
        return getattr(heads, name)
    raise AttributeError(name)


_IMAGES = ("ImageBatch", "preprocess", "random_resized_crop_boxes", "random_flips", "TrainAugment", "collate",
           "ColorItem", "ColorJitter", "color_jitter_u8", "AffineItem", "affine_u8", "rotation_matrix", "affine_matrix",
           "RandomAffine", "RandomRotation", "EnhanceItem", "enhance_u8", "apply_policy_u8", "RandAugment",
           "TrivialAugmentWide")
_EVALUATION = ("RankResult", "target_ranks", "TopK", "topk", "recall_at_k", "rank_summary", "evaluate_retrieval",
               "ClassificationMeter", "ClassificationResult", "classification_report", "accuracy", "evaluate_model",
               "evaluate_enhanced_model", "GroupRankResult", "group_ranks", "topk_relevance", "precision_at_k",
               "average_precision_at_k", "average_precision", "MultiLabelMeter", "MultiLabelResult",
               "evaluate_multilabel")
_HEADS = ("class_bce", "MultiLabelCLIPAdapter", "pos_weight_from_counts")
