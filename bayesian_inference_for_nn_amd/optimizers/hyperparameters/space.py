"""The search space of a hyper-parameter optimizer (the contract of Pyesian/optimizers/hyperparameters/space.py): a named
axis is a Number -- Real or Integer, with inclusive bounds --, a named fixed value a Constant."""


class Parameter:
    """A named hyper-parameter."""

    def __init__(self, name: str):
        self._name = name

    @property
    def name(self) -> str:
        return self._name


class Number(Parameter):
    """A numeric hyper-parameter searched over [lower_bound, upper_bound]."""

    def __init__(self, lower_bound, upper_bound, name: str):
        super().__init__(name)
        self._lower_bound, self._upper_bound = lower_bound, upper_bound

    @property
    def lower_bound(self):
        return self._lower_bound

    @property
    def upper_bound(self):
        return self._upper_bound


class Real(Number):
    """A real-valued axis."""


class Integer(Number):
    """An integer-valued axis."""


class Constant(Parameter):
    """A value no optimizer changes (it makes no axis)."""

    def __init__(self, value, name: str):
        super().__init__(name)
        self._value = value

    @property
    def value(self):
        return self._value
