"""The PHYRE task-success readout and its factory (API of slotformer/phyre_planning/models/__init__.py)."""
from ...host.registry import ModelTable
from .readout import PHYREReadout

_TABLE = ModelTable().add('PHYREReadout', PHYREReadout, readout_dict='readout_dict')


def build_model(params):
    """params.model == 'PHYREReadout' -> the model (NotImplementedError else)."""
    return _TABLE.build(params)
