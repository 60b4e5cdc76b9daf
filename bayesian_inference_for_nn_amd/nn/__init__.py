from .BayesianModel import BayesianModel
from .model import ConvNet, DenseNet, conv_sequential_json, model_from_json, sequential_json
