"""DatasetEvaluator, DatasetEvaluators and the plain inference loop (detectron2/evaluation/evaluator.py:
DatasetEvaluator :15-55, DatasetEvaluators :64-98, inference_on_dataset :85-157 without its logging and timing)."""
from collections import OrderedDict

import torch


class DatasetEvaluator:
    """reset() / process(inputs, outputs) per batch / evaluate() at the end, as the reference's base class."""

    def reset(self):
        pass

    def process(self, inputs, outputs):
        pass

    def evaluate(self):
        pass


class DatasetEvaluators(DatasetEvaluator):
    """Several evaluators fed with every batch; evaluate() merges their result dictionaries (None results are left
    out) and refuses a key that two of them produce."""

    def __init__(self, evaluators):
        self._evaluators = list(evaluators)

    def reset(self):
        for e in self._evaluators:
            e.reset()

    def process(self, inputs, outputs):
        for e in self._evaluators:
            e.process(inputs, outputs)

    def evaluate(self):
        merged = OrderedDict()
        for e in self._evaluators:
            for key, value in (e.evaluate() or {}).items():
                assert key not in merged, "two evaluators produce results under the key %r" % (key,)
                merged[key] = value
        return merged


def inference_on_dataset(model, data_loader, evaluator):
    """Run `model` in eval mode under torch.no_grad() over `data_loader`, feed every batch to `evaluator` and return
    evaluator.evaluate() ({} when that returns None, as the reference).  The model's mode is restored."""
    evaluator.reset()
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for inputs in data_loader:
                evaluator.process(inputs, model(inputs))
    finally:
        model.train(was_training)
    results = evaluator.evaluate()
    return {} if results is None else results
