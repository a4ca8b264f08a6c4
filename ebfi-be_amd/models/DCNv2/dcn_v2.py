"""Drop-in for `models.DCNv2.dcn_v2`: the deformable convolution and the deformable PS-ROI pooling (no ONNX wrapper)."""
from ebfi_amd.dcn import DCN, DCN_sep, DCNv2, _DCNv2, dcn_v2_conv  # noqa: F401
from ebfi_amd.dcn import DCNPooling, DCNv2Pooling, _DCNv2Pooling, dcn_v2_pooling  # noqa: F401
from ebfi_amd.dcn import dcn_v2_pooling_backward, dcn_v2_pooling_forward  # noqa: F401
