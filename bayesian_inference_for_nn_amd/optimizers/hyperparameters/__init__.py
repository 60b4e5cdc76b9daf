from .HyperParameters import HyperParameters
from .space import Parameter, Number, Real, Integer, Constant
from .HyperparameterOptimizer import HyperparameterOptimizer
from .GridOptimizer import GridOptimizer, SGLDGridObjective, BBBGridObjective
