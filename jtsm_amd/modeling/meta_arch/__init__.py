from .build import META_ARCH_REGISTRY, build_model
from .mcnn import GeneralizedMCNNWSL
from .rcnn import GeneralizedRCNN, PanopticFPN
from .rcnn_wsl import GeneralizedRCNNWSL
from .retinanet import RetinaNet, RetinaNetHead
from .semantic_seg import SEM_SEG_HEADS_REGISTRY, SemanticSegmentor, SemSegFPNHead, build_sem_seg_head
from .deeplab import DeepLabV3Head, DeepLabV3PlusHead
from .panoptic_deeplab import (INS_EMBED_BRANCHES_REGISTRY, PanopticDeepLab, PanopticDeepLabInsEmbedHead,
                               PanopticDeepLabSemSegHead, build_ins_embed_branch)
