"""`models` namespace of the SV family (the reference exports the same names from models/__init__.py:6-9) and of its vector-neuron
baselines (the reference's models/vn_dgcnn_cls.py, models/vn_dgcnn_partseg.py, models/vn_pointnet_cls.py and
models/vn_pointnet_partseg.py), and its binary baseline BiPointNet_CLS (the reference's models/bipointnet.py: BiPointNetLSREMax, as
its models/__init__.py names it)."""
from .sv_dgcnn_cls import SV_DGCNN_CLS
from .sv_dgcnn_partseg import SV_DGCNN_PSEG
from .sv_pointnet_cls import SV_PointNet_CLS
from .sv_pointnet_partseg import SV_PointNet_PSEG
from .vn_dgcnn_cls import VN_DGCNN_CLS
from .vn_dgcnn_partseg import VN_DGCNN_PSEG
from .vn_pointnet_cls import VN_PointNet_CLS
from .vn_pointnet_partseg import VN_PointNet_PSEG
from .bipointnet import BiPointNetLSREMax as BiPointNet_CLS

__all__ = ["SV_DGCNN_CLS", "SV_DGCNN_PSEG", "SV_PointNet_CLS", "SV_PointNet_PSEG", "VN_DGCNN_CLS", "VN_DGCNN_PSEG", "VN_PointNet_CLS",
           "VN_PointNet_PSEG", "BiPointNet_CLS"]
