"""What the host tests read out of the C headers under include/."""
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def header_text(name):
    return open(os.path.join(INCLUDE, name)).read()


def declared_symbols(name):
    """the functions that header ``name`` declares, sorted"""
    text = re.sub(r"/\*.*?\*/", "", header_text(name), flags=re.S)
    return sorted(set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", text)))


def macros(name):
    """{macro: value} of every ``#define PS_*`` of header ``name`` whose value is one integer or float literal"""
    found = re.findall(r"^#define (PS_[A-Z0-9_]+)[ \t]+(\d+|\d+\.\d*f?)[ \t]*(?:/\*.*)?$", header_text(name), flags=re.M)
    return {macro: int(text) if text.isdigit() else float(text.rstrip("f")) for macro, text in found}


def parameters(name, symbol):
    """the parameters header ``name`` declares for ``symbol``, as written (``(void)``: none)"""
    text = re.sub(r"/\*.*?\*/", "", header_text(name), flags=re.S)
    listed = re.search(r"\b" + symbol + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    return [] if listed.strip() == "void" else [" ".join(p.split()) for p in listed.split(",")]
