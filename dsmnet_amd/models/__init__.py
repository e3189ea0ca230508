"""Model factory with the reference's interface (models/__init__.py:4-34).

The five networks whose files exist in the reference are built here: ``dispnet`` (no cost volume) and the
four on the cost-volume path.  The ``*_m1/_m2`` names (whose files are absent from the reference too) raise."""

dict_models = ["dispnet", "dispnetcorr", "iresnet", "gcnet", "psmnet"]


def model_create_by_name(name_model, maxdisparity=192):
    if name_model == "psmnet":
        from .psmnet.stackhourglass import PSMNet
        return PSMNet(maxdisparity)
    if name_model == "gcnet":
        from .gcnet import gcnet
        return gcnet(maxdisparity)
    if name_model == "dispnet":
        from .dispnet import dispnet
        return dispnet(maxdisparity)
    if name_model == "dispnetcorr":
        from .dispnetcorr import dispnetcorr
        return dispnetcorr(maxdisparity)
    if name_model == "iresnet":
        from .iresnet import iresnet
        return iresnet(maxdisparity)
    raise AssertionError("model %r is not built on the MI355X path" % (name_model,))
