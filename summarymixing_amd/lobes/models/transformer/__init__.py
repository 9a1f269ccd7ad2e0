from .TransformerLM import TransformerLM  # noqa: F401
