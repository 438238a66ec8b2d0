"""The Physion VQA readout and its factory (API of slotformer/physion_vqa/models/__init__.py)."""
from ...host.registry import ModelTable
from .readout import PhysionReadout

_TABLE = ModelTable().add('PhysionReadout', PhysionReadout, readout_dict='readout_dict')


def build_model(params):
    """params.model == 'PhysionReadout' -> the model (NotImplementedError else)."""
    return _TABLE.build(params)
