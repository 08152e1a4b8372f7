'use strict';
// Device context: the object passed where the reference passes its WebGL2RenderingContext (`gl`,
// RenderingContext.js:66-106).
const { native } = require('./native.js');
const R = require('./readers/readers.js');

// what gl.getExtension('EXT_texture_norm16') returns in WebGL2: the extension's sized internal formats
function norm16Extension() {
    return Object.freeze({
        R16_EXT: R.GL_R16_EXT, RG16_EXT: R.GL_RG16_EXT, RGB16_EXT: R.GL_RGB16_EXT, RGBA16_EXT: R.GL_RGBA16_EXT,
        R16_SNORM_EXT: R.GL_R16_SNORM_EXT, RG16_SNORM_EXT: R.GL_RG16_SNORM_EXT, RGB16_SNORM_EXT: R.GL_RGB16_SNORM_EXT,
        RGBA16_SNORM_EXT: R.GL_RGBA16_SNORM_EXT,
    });
}
const EXTENSIONS = { EXT_texture_norm16: norm16Extension };

class Context {
    constructor(device) {
        this.device = device === undefined ? 0 : device;
        this._h = native().contextCreate(this.device);
        this._extensions = {};
    }
    // WebGL's getExtension: the extension object (enabled on this context from now on), or null for a name this library does not know
    getExtension(name) {
        if (!Object.prototype.hasOwnProperty.call(EXTENSIONS, name)) { return null; }
        if (!this._extensions[name]) { this._extensions[name] = EXTENSIONS[name](); }
        return this._extensions[name];
    }
    extensionEnabled(name) { return Object.prototype.hasOwnProperty.call(this._extensions, name); }
    static deviceCount() { return native().deviceCount(); }
    synchronize() { native().contextSynchronize(this._h); }
    destroy() { if (this._h) { native().contextDestroy(this._h); this._h = null; } }
}
module.exports = { Context };
