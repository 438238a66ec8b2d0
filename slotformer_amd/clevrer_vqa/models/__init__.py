"""The Aloe VQA model and its factory (API of slotformer/clevrer_vqa/models/__init__.py)."""
from nerv.utils import load_obj

from .aloe import CLEVRERAloe
from .transformer import CLEVRERTransformerModel, AloeEncoder, remap_encoder_keys


def build_transformer(params):
    """params.vocab_file names the vocabulary ({'q_vocab': [...], 'a_vocab': [...]}); its sizes are the only thing read from it."""
    vocab = load_obj(params.vocab_file)
    lang_dict = dict(question_vocab_size=len(vocab['q_vocab']), answer_vocab_size=len(vocab['a_vocab']), question_len=params.max_question_len)
    return CLEVRERTransformerModel(transformer_dict=params.transformer_dict, lang_dict=lang_dict, vision_dict=params.vision_dict,
                                   loss_dict=params.loss_dict)


def build_model(params):
    """params.model == 'CLEVRERAloe' -> the model (NotImplementedError else)."""
    if params.model != 'CLEVRERAloe':
        raise NotImplementedError(f'{params.model} is not implemented.')
    return CLEVRERAloe(transformer_model=build_transformer(params))
