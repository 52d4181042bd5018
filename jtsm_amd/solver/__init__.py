from .build import SGD, Adam, build_optimizer  # noqa: F401
