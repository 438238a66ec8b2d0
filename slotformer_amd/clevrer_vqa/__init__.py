"""slotformer.clevrer_vqa counterpart: build_model and the host assembly of the result records test_clevrer_vqa.py writes.  Inference only; the
loop itself is `harness.clevrer_answers`."""
import numpy as np

from .models import build_model, CLEVRERAloe, CLEVRERTransformerModel

FIRST_TEST_SCENE = 15000   # test_clevrer_vqa.py: results[scene_index - 15000]
NUM_TEST_SCENES = 5000


def build_dataset(params, *a, **k):
    raise NotImplementedError('datasets are host-side I/O outside the hot path (SURVEY.md 2.1 row 13)')


def build_method(*a, **k):
    raise NotImplementedError('the nerv trainer is outside the hot path (SURVEY.md 2.1 row 12); the training kernels of CLEVRERAloe are not built')


def result_records(cls_answers, mc_answers, questions, label2answer, first_scene=FIRST_TEST_SCENE, num_scenes=NUM_TEST_SCENES):
    """The list test_clevrer_vqa.py dumps as CLEVRER.json, from the answers of `harness.clevrer_answers`.

    cls_answers [B1] answer ids and mc_answers [Bn] booleans; questions: the collated arrays `cls_scene_index`, `cls_question_id` [B1],
    `mc_scene_index`, `mc_question_id` [B2], `mc_flag`, `mc_choice_id` [Bn]; label2answer: id -> answer word.  Descriptive questions get
    {'question_id', 'answer'}; the choices of a multiple-choice question get {'choice_id', 'answer': 'correct' | 'wrong'} under one
    {'question_id', 'choices'} entry per question -- a question id already present in its scene is extended, as there."""
    results = [{'scene_index': i + first_scene, 'questions': []} for i in range(num_scenes)]
    cls_answers, mc_answers = np.asarray(cls_answers).reshape(-1), np.asarray(mc_answers).reshape(-1).astype(bool)
    for i in range(cls_answers.size):
        results[int(questions['cls_scene_index'][i]) - first_scene]['questions'].append(
            {'question_id': int(questions['cls_question_id'][i]), 'answer': str(label2answer[int(cls_answers[i])])})
    flag, choice_id = np.asarray(questions['mc_flag']).reshape(-1), np.asarray(questions['mc_choice_id']).reshape(-1)
    for i in range(len(questions['mc_question_id'])):
        q_id = int(questions['mc_question_id'][i])
        sel = flag == i
        choices = [{'choice_id': int(c), 'answer': 'correct' if a else 'wrong'} for c, a in zip(choice_id[sel], mc_answers[sel])]
        q_list = results[int(questions['mc_scene_index'][i]) - first_scene]['questions']
        for entry in q_list:
            if entry['question_id'] == q_id:
                entry['choices'] += choices
                break
        else:
            q_list.append({'question_id': q_id, 'choices': choices})
    return results
